"""CPU: the flow-field network port (sin_inn_amd/flownet.py) against fixtures written by the reference's own model.py
(tests/golden/make_golden_flownet.py), and the float64 restatement of the network that tests/test_gpu_flownet.py measures the
kernels with (tests/flownet_refs.py: oracle/ is not to change).
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_refs import net_tensors, own_gates, restate  # noqa: E402

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
    forced = restate(name, bufs, w64, times, ys, xs, SCALE, torch.float64, gates=own_gates(name, bufs, w64, times, ys, xs))
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
    assert lib.sininn_flownet_forward(C.byref(a), None, None) != 0          # no grid, no pointers: refused before any launch
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


def test_registry_is_the_union_of_the_five_dicts_and_agrees_with_the_library():
    """the twelve names of `all_model_dict` are the disjoint union of the five dicts; the library supports each model's own
    (encoding, progressive, enc_dim) and refuses it one feature off either way or as encoding 2, which is none of the library's"""
    from sin_inn_amd import _lib, flownet
    views = (flownet.model_dict, flownet.progressive_model_dict, flownet.learnable_model_dict, flownet.grid_model_dict,
             flownet.positional_model_dict)
    union = {}
    for view in views:
        union.update(view)
    assert sum(len(view) for view in views) == len(union) == len(flownet.all_model_dict) == 12
    assert union == flownet.all_model_dict
    lib = _lib.lib()
    for name, cls in flownet.all_model_dict.items():
        net = cls(flownet.ModelParams())
        assert net.is_progressive == (name in ('PRBF', 'PFF', 'PUFF', 'PRFF', 'PRBFG', 'PPE')), name
        a = _lib.FlowNetArgs()
        a.hidden, a.layers, a.out_dim = 256, 3, 4
        a.encoding, a.progressive, a.enc_dim = net.encode.kind, int(net.is_progressive), net.encoding_dim
        assert lib.sininn_flownet_supported(C.byref(a)) == 1, name
        for off in (-1, 1):
            a.enc_dim = net.encoding_dim + off
            assert lib.sininn_flownet_supported(C.byref(a)) == 0, (name, off)
        a.enc_dim, a.encoding = net.encoding_dim, 2
        assert lib.sininn_flownet_supported(C.byref(a)) == 0, name
