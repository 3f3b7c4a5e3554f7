"""CPU: the SIREN flow network (SineLayer / SirenModel of sin_inn_amd/flownet.py) against a fixture written by the reference's own
model.py (tests/golden/make_golden_flownet_siren.py), the float64 restatement that tests/test_gpu_flownet_siren.py measures the kernels
with (`siren_restate` of tests/siren_refs.py), and the C ABI of csrc/siren.hip: sininn_siren_args is index 9 of sininn_sizeof, every
refusal comes before any launch.
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
from siren_refs import siren_restate, siren_tensors  # noqa: E402

SEED = 1111
TIMES, GH, GW, SCALE, STRIDE = (0.0, 0.5), 21, 28, 3.0, 97
KEYS = [f'model.{i}.linear.{s}' for i in range(4) for s in ('weight', 'bias')] + ['model.4.weight', 'model.4.bias']
SHAPES = [(256, 3), (256,)] + 3 * [(256, 256), (256,)] + [(4, 256), (4,)]


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_siren.npz'))


def build():
    from sin_inn_amd import flownet
    torch.manual_seed(SEED)
    return flownet.SirenModel(flownet.ModelParams())


def fixture_axes():
    return torch.tensor(TIMES), torch.linspace(-1, 1, GH), torch.linspace(-1, 1, GW)


def test_port_holds_the_reference_numbers(gold):
    from sin_inn_amd import flownet
    net = build()
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold['keys']] == KEYS
    assert [k for k, _ in net.named_parameters()] == KEYS
    for key, shape in zip(KEYS, SHAPES):
        flat = sd[key].detach().reshape(-1)
        assert tuple(sd[key].shape) == shape, key
        assert np.array_equal(flat[:32].numpy(), gold[f'head_{key}']), key
        assert np.array_equal(flat[-32:].numpy(), gold[f'tail_{key}']), key
        assert flat.double().sum().item() == float(gold[f'sum_{key}']), key
    assert net.is_progressive is False and net.encoding_dim == 3 and net.domain_dim == 3 and net.omega == 30.0
    assert net.update_progress() is None and net.stash_iteration(torch.tensor(0.5)) is None
    lins = net.linears()
    assert len(lins) == 5 and all(isinstance(m, torch.nn.Linear) for m in lins)
    assert all(a is b for a, b in zip([p for lin in lins for p in (lin.weight, lin.bias)], net.parameters()))
    first = net.model[0]
    assert isinstance(first, flownet.SineLayer) and first.is_first and first.omega_0 == 30 and first.in_features == 3
    assert isinstance(net.model[4], torch.nn.Linear)
    with pytest.raises(NotImplementedError):
        net(torch.zeros(7, 3))


def test_restatement_reproduces_the_reference(gold):
    weights = siren_tensors(build())
    times, ys, xs = fixture_axes()
    w64 = [p.double().requires_grad_(True) for p in weights]
    flows = siren_restate(w64, times, ys, xs, SCALE, torch.float64)
    ref = torch.from_numpy(gold['out64'])
    assert float((flows.detach() - ref).abs().max() / ref.abs().max()) < 1e-12
    with torch.no_grad():
        f32 = siren_restate(weights, times, ys, xs, SCALE, torch.float32)
    ref32 = torch.from_numpy(gold['out32'])
    assert float((f32 - ref32).abs().max() / ref32.abs().max()) < 1e-4       # two fp32 evaluations (thread count, BLAS blocking)
    grads = torch.autograd.grad((flows * torch.from_numpy(gold['up']).double()).sum(), w64)
    for key, shape, g in zip(KEYS, SHAPES, grads):
        assert tuple(g.shape) == shape
        g = g.reshape(-1)
        sub = g if g.numel() <= 8192 else g[::STRIDE]
        want = torch.from_numpy(gold[f'gsub_{key}'])
        assert float((sub - want).abs().max()) <= 1e-12 * float(want.abs().max()), key
        gabs = float(gold[f'gabs_{key}'])
        assert abs(g.sum().item() - float(gold[f'gsum_{key}'])) <= 1e-12 * gabs, key
        assert abs(g.abs().sum().item() - gabs) <= 1e-12 * gabs, key


def test_omega_is_a_factor_of_the_weights():
    """the identity the GPU test uses to show that omega is a run-time argument: omega = 1 with 30 W_l, 30 b_l (l = 1 .. 4) has the same phases"""
    weights = [p.double() for p in siren_tensors(build())]
    times, ys, xs = fixture_axes()
    scaled = [p * 30 for p in weights[:8]] + weights[8:]
    a = siren_restate(weights, times, ys, xs, SCALE, torch.float64)
    b = siren_restate(scaled, times, ys, xs, SCALE, torch.float64, omega=1.0)
    assert float((a - b).abs().max() / a.abs().max()) < 1e-12


def test_abi_and_refusals():
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'sininn.h')).read()
    for sym in ('sininn_siren_supported', 'sininn_siren_saved_bytes', 'sininn_siren_workspace_bytes', 'sininn_siren_forward',
                'sininn_siren_backward'):
        assert hasattr(lib, sym) and sym in _lib.EXPORTED and sym + '(' in header, sym
    assert lib.sininn_sizeof(9) == C.sizeof(_lib.SirenArgs) and lib.sininn_sizeof(9) > 0
    assert lib.sininn_sizeof(7) == 280 == C.sizeof(_lib.FlowNetArgs)
    assert lib.sininn_sizeof(10) == C.sizeof(_lib.FlowNetCall) and lib.sininn_sizeof(11) == 0 and lib.sininn_version() == 4
    for sym in ('sininn_siren_forward_points', 'sininn_siren_backward_points', 'sininn_siren_backward_posegrad_points'):
        assert sym not in _lib.EXPORTED and not hasattr(lib, sym) and sym + '(' not in header, sym

    def fresh():
        a = _lib.SirenArgs()
        a.in_dim, a.hidden, a.layers, a.out_dim, a.omega = 3, 256, 3, 4, 30.0
        return a
    a = fresh()
    assert a.struct_bytes == C.sizeof(_lib.SirenArgs) and lib.sininn_siren_supported(C.byref(a)) == 1
    # ---- struct_bytes ----
    a.struct_bytes -= 8
    assert lib.sininn_siren_supported(C.byref(a)) == 0
    for call in (lib.sininn_siren_forward, lib.sininn_siren_backward):
        assert call(C.byref(a), None, None) != 0 and b'struct_bytes' in lib.sininn_last_error()
    # ---- sizes and omega: the message names what the library is built for ----
    for field, value in (('hidden', 128), ('layers', 2), ('in_dim', 2), ('out_dim', 2), ('omega', 0.0), ('omega', -30.0),
                         ('omega', float('inf')), ('omega', float('nan'))):
        a = fresh()
        setattr(a, field, value)
        a.T, a.H, a.W = 2, 8, 8
        assert lib.sininn_siren_supported(C.byref(a)) == 0, (field, value)
        for call in (lib.sininn_siren_forward, lib.sininn_siren_backward):
            assert call(C.byref(a), None, None) != 0, (field, value)
            msg = lib.sininn_last_error()
            assert b'built for 3 -> 256 x (1 + 3) -> 4' in msg and b'omega > 0' in msg, msg
    # ---- sizes of the buffers ----
    assert lib.sininn_siren_saved_bytes(0) == 0 and lib.sininn_siren_workspace_bytes(0) == 0
    assert lib.sininn_siren_saved_bytes(1) == lib.sininn_siren_saved_bytes(64) == 4 * 64 * 256 * 4
    assert lib.sininn_siren_saved_bytes(65) == 4 * 128 * 256 * 4
    assert lib.sininn_siren_workspace_bytes(64) > 6 * 64 * 256 * 4 + 3 * 256 * 256 * 4
    assert lib.sininn_siren_workspace_bytes((1 << 22) + 1) == 0
    # ---- grid, null and short buffers: host memory stands in, nothing is launched ----
    n = 2 * 8 * 8
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p)

    def filled():
        a = fresh()
        a.T, a.H, a.W, a.scale = 2, 8, 8, 1.0
        a.times = a.ys = a.xs = p
        for l in range(5):
            a.w[l] = a.b[l] = a.gw[l] = a.gb[l] = p
        a.flows = a.dflows = a.saved = a.workspace = p
        a.saved_bytes, a.workspace_bytes = lib.sininn_siren_saved_bytes(n), lib.sininn_siren_workspace_bytes(n)
        return a
    a = filled()
    a.T = 0
    assert lib.sininn_siren_forward(C.byref(a), None, None) != 0 and b'grid' in lib.sininn_last_error()
    a = filled()
    a.T, a.H, a.W = 1 << 10, 1 << 10, 8
    assert lib.sininn_siren_forward(C.byref(a), None, None) != 0 and b'grid' in lib.sininn_last_error()
    a = filled()
    a.flows = None
    assert lib.sininn_siren_forward(C.byref(a), None, None) != 0 and b'null flows' in lib.sininn_last_error()
    a = filled()
    a.w[2] = None
    assert lib.sininn_siren_forward(C.byref(a), None, None) != 0 and b'null weight' in lib.sininn_last_error()
    a = filled()
    a.saved_bytes -= 4
    assert lib.sininn_siren_forward(C.byref(a), None, None) != 0 and b'saved holds' in lib.sininn_last_error()
    assert lib.sininn_siren_backward(C.byref(a), None, None) != 0 and b'saved holds' in lib.sininn_last_error()
    a = filled()
    a.workspace_bytes -= 4
    assert lib.sininn_siren_backward(C.byref(a), None, None) != 0 and b'workspace holds' in lib.sininn_last_error()
    a = filled()
    a.dflows = None
    assert lib.sininn_siren_backward(C.byref(a), None, None) != 0 and b'null dflows' in lib.sininn_last_error()
    a = filled()
    a.gb[4] = None
    assert lib.sininn_siren_backward(C.byref(a), None, None) != 0 and b'null gradient' in lib.sininn_last_error()


def test_registry_and_command_line_stay_as_they_are(capsys):
    from sin_inn_amd import flownet
    assert len(flownet.all_model_dict) == 12 and 'siren' not in flownet.all_model_dict
    assert flownet.siren_model_dict == {'siren': flownet.SirenModel}
    spec = importlib.util.spec_from_file_location('flow_main_siren', os.path.join(ROOT, 'video-interpolation', 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.OUT_OF_SCOPE_NETWORKS == ('siren', 'MPFF') and len(m.NETWORKS) == 12
    with pytest.raises(SystemExit) as e:
        m.get_args(['train', '--net', 'siren'])
    assert e.value.code == 2 and 'out of scope' in capsys.readouterr().err


def test_cpu_tensors_and_other_sizes_are_refused():
    from sin_inn_amd import flownet
    net = build()
    with pytest.raises(NotImplementedError):
        flownet.flow_fields(net, torch.tensor([0.0, 0.5]), 8, 8, 1.0)
    fake = torch.zeros(2)
    for kw in (dict(hidden_dim=128), dict(num_layers=2), dict(domain_dim=2), dict(output_channels=2)):
        with pytest.raises(ValueError, match='built for 3 -> 256'):
            flownet._siren_args(flownet.SirenModel(flownet.ModelParams(**kw)), fake, fake, fake, 1.0)
    with pytest.raises(ValueError, match='omega > 0'):
        flownet._siren_args(net, fake, fake, fake, 1.0, omega=0.0)
    with pytest.raises(NotImplementedError):
        flownet._siren_args(net, fake, fake, fake, 1.0)          # supported sizes, CPU axis vectors


def test_state_dict_round_trip():
    from sin_inn_amd import flownet
    net = build()
    other = flownet.SirenModel(flownet.ModelParams())
    with torch.no_grad():
        for p in other.parameters():
            p.zero_()
    other.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    for (ka, va), (kb, vb) in zip(net.state_dict().items(), other.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
