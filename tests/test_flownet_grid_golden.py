"""CPU: the radial-basis-grid flow-field networks RBFG / PRBFG (sin_inn_amd/flownet.py) against a fixture written by the reference's
own model.py and progressive_controller.py (tests/golden/make_golden_flownet_grid.py), and the float64 restatement of the encoding
and the network that tests/test_gpu_flownet_grid.py measures the kernels with (`encode_grid`, `restate` of tests/flownet_refs.py).
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_refs import net_tensors, own_gates, restate  # noqa: E402

NETS = ('RBFG', 'PRBFG')
SEED = {'RBFG': 707, 'PRBFG': 808}
TIMES, GH, GW, SCALE, STRIDE = (0.0, 0.5), 20, 28, 3.0, 97
MAX_ITERATION, EPSILON, N_RAMP, N_MID = 1000, 1e-3, 98, 100
KEYS = [f'model.model.{i}.{s}' for i in (0, 2, 4, 6) for s in ('weight', 'bias')]


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_grid.npz'))


def build(name):
    from sin_inn_amd import flownet
    torch.manual_seed(SEED[name])
    return flownet.grid_model_dict[name](flownet.ModelParams())


def controller(net):
    from sin_inn_amd import progressive
    return progressive.LinearControllerEarly(net, MAX_ITERATION, epsilon=EPSILON)


def flow_main():
    spec = importlib.util.spec_from_file_location('flow_main_grid', os.path.join(ROOT, 'video-interpolation', 'main.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('name', NETS)
def test_port_holds_the_reference_numbers(gold, name):
    net = build(name)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold[f'{name}_keys']]
    assert list(sd.keys())[:2] == ['encode.offsets', 'encode.sigma']
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
    prog = name == 'PRBFG'
    assert net.encode.kind == 3 and net.encode.output_channels == 512 and net.domain_dim == 3
    assert net.is_progressive == prog and net.encoding_dim == (515 if prog else 512)
    assert tuple(sd['model.model.0.weight'].shape) == (256, 515 if prog else 512) and tuple(sd['model.model.6.weight'].shape) == (4, 256)
    offsets, sigma = net.encode.kernel_buffers()
    assert tuple(offsets.shape) == (256, 3) and tuple(sigma.shape) == (256,) and offsets.dtype == sigma.dtype == torch.float32
    assert bool((sigma[1:] > sigma[:-1]).all()) and bool((offsets >= 0).all()) and bool((offsets <= 2 / sigma[:, None]).all())
    with pytest.raises(NotImplementedError):
        net(torch.zeros(4, 3))


def test_restatement_reproduces_the_reference_rbfg(gold):
    name = 'RBFG'
    net = build(name)
    bufs, weights = net_tensors(net)
    times, ys, xs = torch.tensor(TIMES), torch.linspace(-1, 1, GH), torch.linspace(-1, 1, GW)
    w64 = [p.double().requires_grad_(True) for p in weights]
    flows = restate(name, bufs, w64, times, ys, xs, SCALE, torch.float64)
    ref = torch.from_numpy(gold[f'{name}_out64'])
    assert float((flows.detach() - ref).abs().max() / ref.abs().max()) < 1e-12
    with torch.no_grad():
        f32 = restate(name, bufs, weights, times, ys, xs, SCALE, torch.float32)
    ref32 = torch.from_numpy(gold[f'{name}_out32'])
    assert float((f32 - ref32).abs().max() / ref32.abs().max()) < 1e-4      # two fp32 evaluations (thread count, BLAS blocking)
    forced = restate(name, bufs, w64, times, ys, xs, SCALE, torch.float64, None, own_gates(name, bufs, w64, times, ys, xs, None))
    assert float((forced.detach() - ref).abs().max() / ref.abs().max()) < 1e-12
    check_grads(gold, name, torch.autograd.grad((forced * torch.from_numpy(gold['up']).double()).sum(), w64), None)


def test_restatement_reproduces_the_reference_prbfg(gold):
    name = 'PRBFG'
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
            assert float((f32 - ref32).abs().max() / ref32.abs().max()) < 1e-4, k
    mask = masks['ramp']
    forced = restate(name, bufs, w64, times, ys, xs, SCALE, torch.float64, mask, own_gates(name, bufs, w64, times, ys, xs, mask))
    ref = torch.from_numpy(gold[f'{name}_out64_ramp'])
    assert float((forced.detach() - ref).abs().max() / ref.abs().max()) < 1e-12
    check_grads(gold, name, torch.autograd.grad((forced * torch.from_numpy(gold['up']).double()).sum(), w64), mask)


def check_grads(gold, name, grads, mask):
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
        if mask is not None and key == 'model.model.0.weight':
            want = torch.from_numpy(gold[f'{name}_gcoord'])
            assert float((full[:, :3] - want).abs().max()) <= 1e-12 * float(want.abs().max())
            assert float(want.abs().max()) > 0 and bool((full[:, mask == 0] == 0).all())


def test_controller_wraps_prbfg_unchanged(gold):
    ctl = controller(build('PRBFG'))
    assert ctl.is_progressive and ctl.encoding_dim == 515 and ctl.domain_dim == 3 and ctl.block_size == 6
    for i in range(N_MID):
        ctl.stash_iteration(torch.tensor(0.5))
        if i + 1 == N_RAMP:
            assert np.array_equal(ctl.mask.numpy(), gold['mask_ramp'])
    assert np.array_equal(ctl.mask.numpy(), gold['mask_mid'])
    with pytest.raises(NotImplementedError):
        ctl(torch.zeros(4, 3))


def test_abi_and_refusals():
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, flownet
    lib = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'sininn.h')).read()
    assert '#define SININN_FLOWNET_RBFG 3' in header and flownet.RBFG == 3
    assert lib.sininn_sizeof(7) == 280 == C.sizeof(_lib.FlowNetArgs)
    a = _lib.FlowNetArgs()
    a.encoding, a.hidden, a.layers, a.out_dim = 3, 256, 3, 4
    for enc_dim, progressive, want in ((512, 0, 1), (515, 1, 1), (515, 0, 0), (512, 1, 0)):
        a.enc_dim, a.progressive = enc_dim, progressive
        assert lib.sininn_flownet_supported(C.byref(a)) == want, (enc_dim, progressive)
    a.enc_dim, a.progressive = 512, 0
    assert lib.sininn_flownet_encgrad_workspace_bytes(C.byref(a)) == 0
    g = (C.c_float * 768)()
    rc = lib.sininn_flownet_backward(C.byref(a), C.byref(_lib.FlowNetCall(mode=_lib.ENCGRAD, g_enc_a=C.cast(g, C.c_void_p))), None)    # refused on the encoding, before any launch
    assert rc != 0 and b'SININN_FLOWNET_FOURIER' in lib.sininn_last_error()
    a.T, a.H, a.W = 2, 8, 8
    assert lib.sininn_flownet_forward(C.byref(a), None, None) != 0                  # no pointers: refused before any launch
    assert b'null' in lib.sininn_last_error()
    a.hidden = 128
    assert lib.sininn_flownet_forward(C.byref(a), None, None) != 0
    assert b'RBFG' in lib.sininn_last_error()
    assert flownet.grid_model_dict == {'RBFG': flownet.RbfgModel, 'PRBFG': flownet.PRBFGModel}
    for name in NETS:
        with pytest.raises(NotImplementedError):
            flownet.flow_fields(build(name), torch.tensor([0.0, 0.5]), 8, 8, 1.0)
    fake = torch.zeros(2)
    with pytest.raises(ValueError):
        flownet._args(build('PRBFG'), fake, fake, fake, 1.0)                  # a progressive network without a mask
    with pytest.raises(ValueError):
        flownet._args(flownet.RbfgModel(flownet.ModelParams(hidden_dim=128)), fake, fake, fake, 1.0)


@pytest.mark.parametrize('name', NETS)
def test_command_line_takes_the_grid_networks(name):
    from sin_inn_amd import flownet, progressive
    m = flow_main()
    args = m.get_args(['train', '--net', name])
    assert args.net == name and name in m.NETWORKS and name not in m.OUT_OF_SCOPE_NETWORKS
    net = m.build_net(args)
    assert args.net_name == name
    if name == 'PRBFG':
        assert isinstance(net, progressive.LinearControllerEarly) and isinstance(net.model, flownet.PRBFGModel)
        assert net.encoding_dim == 515 and net.block_size == 6
    else:
        assert isinstance(net, flownet.RbfgModel) and net.encoding_dim == 512


@pytest.mark.parametrize('name', NETS)
def test_state_dict_round_trip(name):
    from sin_inn_amd import flownet
    net = build(name)
    other = flownet.grid_model_dict[name](flownet.ModelParams())
    with torch.no_grad():
        for p in other.parameters():
            p.zero_()
        other.encode.offsets.zero_()
        other.encode.sigma.fill_(1.0)
    other.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    for (ka, va), (kb, vb) in zip(net.state_dict().items(), other.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka


def test_state_dict_round_trip_of_a_wrapped_prbfg():
    ctl = controller(build('PRBFG'))
    assert list(ctl.state_dict().keys()) == ['mask_stashed', 'model.encode.offsets', 'model.encode.sigma'] + ['model.' + k for k in KEYS]
    for i in range(N_MID):
        ctl.stash_iteration(torch.tensor(0.5))
    torch.manual_seed(1)
    from sin_inn_amd import flownet
    other = controller(flownet.PRBFGModel(flownet.ModelParams()))
    other.load_state_dict({k: v.clone() for k, v in ctl.state_dict().items()})
    assert torch.equal(ctl.mask, other.mask) and other.mask.shape == (515,)
    for (ka, va), (kb, vb) in zip(ctl.state_dict().items(), other.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
