"""CPU: the flow-field network port (sin_inn_amd/flownet.py) against fixtures written by the reference's own model.py
(tests/golden/make_golden_flownet.py), and the float64 restatement of the network that tests/test_gpu_flownet.py measures the
kernels with.  The restatement lives here because oracle/ is not to change; `restate` is imported by the GPU test.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ('RBF', 'FFN', 'UFF')
SEED = {'RBF': 101, 'FFN': 202, 'UFF': 303}
TIMES, GH, GW, SCALE, STRIDE = (0.0, 0.5), 20, 28, 3.0, 97


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet.npz'))


def build(name):
    from sin_inn_amd import flownet
    torch.manual_seed(SEED[name])
    return flownet.model_dict[name](flownet.ModelParams())


def encode(name, bufs, poses):
    """model.py:349-356 (RBF) / model.py:230-238 (FFN, UFF), in the dtype of `poses`"""
    if name == 'RBF':
        centres, sigma = bufs['encode.centres'].to(poses), bufs['encode.sigma'].to(poses)
        out = (poses[:, None, :] - centres[None, :, :]).pow(2).sum(2)
        return torch.exp(-(out * sigma[None, :] ** 2))
    freq = bufs['encode.frequencies'].to(poses)
    out = torch.matmul(poses * 2 * np.pi, freq)
    return torch.stack((torch.sin(out), torch.cos(out)), dim=2).view(poses.shape[0], -1)


def restate(name, bufs, weights, times, ys, xs, scale, dtype, gates=None):
    """FlowTrainer.forward (trainer.py:37-45) in plain torch in `dtype`, from fp32 axis vectors / buffers / weights (widened).
    weights: [W1, b1, .., W4, b4] (autograd leaves of `dtype` if gradients are wanted); gates: None (ReLU) or three bool
    (N, 256) tensors that REPLACE the ReLU decision: h = pre * gate.  Returns flows (t, 4, h, w)."""
    t, h, w = times.numel(), ys.numel(), xs.numel()
    weights = [p.to(dtype) for p in weights]
    gt, gh, gw = torch.meshgrid(times.to(dtype), ys.to(dtype), xs.to(dtype), indexing='ij')
    poses = torch.stack((gt, gh, gw), dim=-1).view(-1, 3)
    x = encode(name, bufs, poses)
    for l in range(3):
        pre = torch.nn.functional.linear(x, weights[2 * l], weights[2 * l + 1])
        x = torch.relu(pre) if gates is None else pre * gates[l].to(dtype)
    out = torch.nn.functional.linear(x, weights[6], weights[7])
    return out.view(t, h, w, 4).permute(0, 3, 1, 2) * scale


def net_tensors(net, device='cpu'):
    bufs = {k: v.detach().to(device) for k, v in net.state_dict().items() if k.startswith('encode.')}
    weights = [p.detach().to(device) for lin in net.linears() for p in (lin.weight, lin.bias)]
    return bufs, weights


@pytest.mark.parametrize('name', NETS)
def test_port_holds_the_reference_numbers(gold, name):
    net = build(name)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold[f'{name}_keys']]
    params = dict(net.named_parameters())
    assert sorted(params) == sorted(f'model.model.{i}.{s}' for i in (0, 2, 4, 6) for s in ('weight', 'bias'))
    for key, v in sd.items():
        if key in params:
            flat = v.detach().reshape(-1)
            assert np.array_equal(flat[:32].numpy(), gold[f'{name}_head_{key}']), key
            assert np.array_equal(flat[-32:].numpy(), gold[f'{name}_tail_{key}']), key
            assert flat.double().sum().item() == float(gold[f'{name}_sum_{key}']), key
        else:
            assert np.array_equal(v.numpy(), gold[f'{name}_buf_{key}']), key
    assert net.encode.output_channels == 512 and tuple(sd['model.model.0.weight'].shape) == (256, 512)
    assert tuple(sd['model.model.6.weight'].shape) == (4, 256)


@pytest.mark.parametrize('name', NETS)
def test_restatement_reproduces_the_reference_in_float64(gold, name):
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
    # forced gates equal to the ReLU's own decision change nothing
    with torch.no_grad():
        x = None
        gates = []
        t, h, w = len(TIMES), GH, GW
        gt, gh, gw = torch.meshgrid(times.double(), ys.double(), xs.double(), indexing='ij')
        x = encode(name, bufs, torch.stack((gt, gh, gw), dim=-1).view(-1, 3))
        for l in range(3):
            x = torch.relu(torch.nn.functional.linear(x, w64[2 * l], w64[2 * l + 1]))
            gates.append(x > 0)
    forced = restate(name, bufs, w64, times, ys, xs, SCALE, torch.float64, gates)
    assert float((forced.detach() - ref).abs().max() / ref.abs().max()) < 1e-12
    up = torch.from_numpy(gold['up']).double()
    grads = torch.autograd.grad((forced * up).sum(), w64)
    keys = [f'model.model.{i}.{s}' for i in (0, 2, 4, 6) for s in ('weight', 'bias')]
    for key, g in zip(keys, grads):
        g = g.reshape(-1)
        sub = g if g.numel() <= 1024 else g[::STRIDE]
        want = torch.from_numpy(gold[f'{name}_gsub_{key}'])
        scale = float(want.abs().max())
        assert float((sub - want).abs().max()) <= 1e-12 * scale, key
        gabs = float(gold[f'{name}_gabs_{key}'])
        assert abs(g.sum().item() - float(gold[f'{name}_gsum_{key}'])) <= 1e-12 * gabs, key
        assert abs(g.abs().sum().item() - gabs) <= 1e-12 * gabs, key


def test_abi_and_refusals():
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, flownet
    lib = _lib.lib()
    for sym in ('sininn_flownet_supported', 'sininn_flownet_saved_bytes', 'sininn_flownet_workspace_bytes',
                'sininn_flownet_forward', 'sininn_flownet_backward'):
        assert hasattr(lib, sym) and sym in _lib.EXPORTED
    header = open(os.path.join(ROOT, 'include', 'sininn.h')).read()
    import re
    for sym in set(re.findall(r'\b(sininn_flownet_[a-z0-9_]+)\s*\(', header)):
        assert hasattr(lib, sym), sym
    assert lib.sininn_sizeof(7) == C.sizeof(_lib.FlowNetArgs)
    a = _lib.FlowNetArgs()
    a.encoding, a.enc_dim, a.hidden, a.layers, a.out_dim = 0, 512, 256, 3, 4
    assert lib.sininn_flownet_supported(C.byref(a)) == 1
    a.hidden = 128
    assert lib.sininn_flownet_supported(C.byref(a)) == 0
    a.hidden, a.encoding = 256, 2
    assert lib.sininn_flownet_supported(C.byref(a)) == 0
    a.encoding, a.struct_bytes = 1, 8
    assert lib.sininn_flownet_supported(C.byref(a)) == 0
    a.struct_bytes = C.sizeof(_lib.FlowNetArgs)
    assert lib.sininn_flownet_forward(C.byref(a), None) != 0          # no grid, no pointers: refused before any launch
    assert lib.sininn_last_error()
    n = 3 * 109 * 253
    npad = (n + 63) // 64 * 64
    assert lib.sininn_flownet_saved_bytes(n) == 3 * npad * 256 * 4
    assert lib.sininn_flownet_workspace_bytes(n) > lib.sininn_flownet_saved_bytes(n)
    assert lib.sininn_flownet_saved_bytes(0) == 0 and lib.sininn_flownet_workspace_bytes(1 << 40) == 0
    net = build('RBF')
    with pytest.raises(NotImplementedError):
        flownet.flow_fields(net, torch.tensor([0.0, 0.5]), 8, 8, 1.0)
    with pytest.raises(NotImplementedError):
        net(torch.zeros(4, 3))
    assert sorted(flownet.model_dict) == ['FFN', 'RBF', 'UFF']


def test_other_sizes_raise_instead_of_falling_back():
    from sin_inn_amd import flownet
    torch.manual_seed(0)
    net = flownet.RbfModel(flownet.ModelParams(hidden_dim=128))
    fake = torch.zeros(2)
    with pytest.raises(ValueError):
        flownet._args(net, fake, fake, fake, 1.0)
