"""CPU: the positional-encoding flow-field networks PE / PPE (sin_inn_amd/flownet.py) against a fixture written by the reference's own
model.py and progressive_controller.py (tests/golden/make_golden_flownet_pe.py), and the float64 restatement of the encoding and the
network that tests/test_gpu_flownet_pe.py measures the kernels with (`encode_pe`, `restate` of tests/flownet_refs.py).

The reference's PositionalEncoding.forward reshapes through `.view(-1, 21)` and raises unless the number of points is a multiple of
7; the fixture's grid has 1176 = 7 * 168 points.  `encode_pe` is the formula itself and runs for every N.
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
from flownet_refs import encode_pe, net_tensors, own_gates, poses_of, restate  # noqa: E402

NETS = ('PE', 'PPE')
SEED = {'PE': 909, 'PPE': 1010}
TIMES, GH, GW, SCALE, STRIDE = (0.0, 0.5), 21, 28, 3.0, 97
MAX_ITERATION, EPSILON, N_RAMP, N_MID = 1000, 1e-3, 60, 400
KEYS = [f'model.model.{i}.{s}' for i in (0, 2, 4, 6) for s in ('weight', 'bias')]
WIDTH = {'PE': 24, 'PPE': 27}


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_pe.npz'))


def build(name):
    from sin_inn_amd import flownet
    torch.manual_seed(SEED[name])
    return flownet.positional_model_dict[name](flownet.ModelParams())


def controller(net):
    from sin_inn_amd import progressive
    return progressive.LinearControllerEarly(net, MAX_ITERATION, epsilon=EPSILON)


def flow_main():
    spec = importlib.util.spec_from_file_location('flow_main_pe', os.path.join(ROOT, 'video-interpolation', 'main.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fixture_axes():
    return torch.tensor(TIMES), torch.linspace(-1, 1, GH), torch.linspace(-1, 1, GW)


@pytest.mark.parametrize('name', NETS)
def test_port_holds_the_reference_numbers(gold, name):
    net = build(name)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold[f'{name}_keys']]
    assert list(sd.keys()) == ['encode.freqs'] + KEYS
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
    prog = name == 'PPE'
    assert net.encode.kind == 4 and net.encode.output_channels == 24 and net.domain_dim == 3
    assert net.is_progressive == prog and net.encoding_dim == WIDTH[name]
    assert tuple(sd['model.model.0.weight'].shape) == (256, WIDTH[name]) and tuple(sd['model.model.6.weight'].shape) == (4, 256)
    freqs, none = net.encode.kernel_buffers()
    assert none is None and tuple(freqs.shape) == (4,) and freqs.dtype == torch.float32
    pi32 = np.float32(np.pi)
    assert np.array_equal(freqs.numpy(), np.array([pi32, 2 * pi32, 4 * pi32, 8 * pi32], dtype=np.float32))
    with pytest.raises(NotImplementedError):
        net(torch.zeros(7, 3))


def test_encoding_restatement_is_the_reference_bitwise(gold):
    bufs, _ = net_tensors(build('PE'))
    times, ys, xs = fixture_axes()
    enc32 = encode_pe(bufs, poses_of(times, ys, xs, torch.float32))
    assert enc32.dtype == torch.float32 and tuple(enc32.shape) == (1176, 24)
    assert np.array_equal(enc32.numpy(), gold['encoding'])                       # bitwise against the reference's torch fp32
    enc64 = encode_pe(bufs, poses_of(times, ys, xs, torch.float64))
    assert float((enc64 - torch.from_numpy(gold['encoding']).double()).abs().max()) < 4e-6   # half an ulp of 8 pi, and the functions
    # cosines of a frequency before its sines; feature 6 f + d reads coordinate d
    poses = poses_of(times, ys, xs, torch.float64)
    f = bufs['encode.freqs'].double()
    assert torch.equal(enc64[:, 13], torch.cos(f[2] * poses[:, 1])) and torch.equal(enc64[:, 23], torch.sin(f[3] * poses[:, 2]))


@pytest.mark.parametrize('n', [1, 64, 128, 5883])
def test_restatement_runs_where_the_reference_raises(n):
    """N % 7 != 0: the reference's `.view(-1, 21)` raises, the formula does not care"""
    assert n % 7 != 0
    bufs, _ = net_tensors(build('PE'))
    poses = torch.rand(n, 3, generator=torch.Generator().manual_seed(n)) * 2 - 1
    enc = encode_pe(bufs, poses)
    assert tuple(enc.shape) == (n, 24) and bool(torch.isfinite(enc).all())
    assert float((enc[:, :3] ** 2 + enc[:, 3:6] ** 2 - 1).abs().max()) < 1e-6
    with pytest.raises(RuntimeError):
        torch.zeros(n, 4, 6).view(-1, 21)


def test_restatement_reproduces_the_reference_pe(gold):
    name = 'PE'
    net = build(name)
    bufs, weights = net_tensors(net)
    times, ys, xs = fixture_axes()
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


def test_restatement_reproduces_the_reference_ppe(gold):
    name = 'PPE'
    net = build(name)
    bufs, weights = net_tensors(net)
    times, ys, xs = fixture_axes()
    w64 = [p.double().requires_grad_(True) for p in weights]
    masks = {k: torch.from_numpy(gold[f'mask_{k}']) for k in ('mid', 'ramp')}
    masks['ones'] = torch.ones(27)
    for k, mask in masks.items():
        flows = restate(name, bufs, w64, times, ys, xs, SCALE, torch.float64, mask)
        ref = torch.from_numpy(gold[f'{name}_out64_{k}'])
        assert float((flows.detach() - ref).abs().max() / ref.abs().max()) < 1e-12, k
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
        sub = g if g.numel() <= 8192 else g[::STRIDE]
        want = torch.from_numpy(gold[f'{name}_gsub_{key}'])
        scale = float(want.abs().max())
        assert float((sub - want).abs().max()) <= 1e-12 * scale, key
        gabs = float(gold[f'{name}_gabs_{key}'])
        assert abs(g.sum().item() - float(gold[f'{name}_gsum_{key}'])) <= 1e-12 * gabs, key
        assert abs(g.abs().sum().item() - gabs) <= 1e-12 * gabs, key
        if mask is not None and key == 'model.model.0.weight':
            assert tuple(full.shape) == (256, 27) and float(full[:, :3].abs().max()) > 0 and bool((full[:, mask == 0] == 0).all())


def test_controller_reproduces_the_masks_and_the_trace(gold):
    ctl = controller(build('PPE'))
    assert ctl.is_progressive and ctl.encoding_dim == 27 and ctl.domain_dim == 3
    assert ctl.block_size == 6 == int(gold['block_size'])
    assert ctl.block_iterations == 250 == int(gold['block_iterations']) and ctl.progress_iterations == 750 == int(gold['progress_iterations'])
    assert ctl.mask.tolist() == [1.0] * 6 + [0.0] * 21 and (ctl.cur_block, ctl.next_block) == (6, 12)
    trace = []
    for i in range(MAX_ITERATION):
        ctl.stash_iteration(torch.tensor(0.5))
        trace.append((ctl.cur_block, ctl.next_block))
        if i + 1 == N_RAMP:
            assert np.array_equal(ctl.mask.numpy(), gold['mask_ramp'])
        if i + 1 == N_MID:
            assert np.array_equal(ctl.mask.numpy(), gold['mask_mid'])
    assert np.array_equal(np.array(trace, dtype=np.int64), gold['trace'])
    assert trace[248] == (6, 12) and trace[249] == (12, 18) and trace[499] == (18, 27) and trace[749] == (27, 27)
    assert np.array_equal(ctl.mask.numpy(), gold['mask_final']) and bool((ctl.mask == 1).all())
    from sin_inn_amd import flownet
    assert flownet.last_open(torch.from_numpy(gold['mask_ramp'])) == 12 and flownet.last_open(torch.from_numpy(gold['mask_mid'])) == 18
    with pytest.raises(NotImplementedError):
        ctl(torch.zeros(7, 3))


def test_abi_and_refusals():
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, flownet
    lib = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'sininn.h')).read()
    assert '#define SININN_FLOWNET_PE 4' in header and flownet.PE == 4
    assert lib.sininn_sizeof(7) == 280 == C.sizeof(_lib.FlowNetArgs)
    assert lib.sininn_version() == 4
    a = _lib.FlowNetArgs()
    a.hidden, a.layers, a.out_dim = 256, 3, 4
    cases = ((4, 24, 0, 1), (4, 27, 1, 1), (4, 24, 1, 0), (4, 27, 0, 0), (4, 512, 0, 0), (4, 515, 1, 0), (4, 32, 0, 0),
             (0, 24, 0, 0), (1, 24, 0, 0), (3, 24, 0, 0), (0, 27, 1, 0), (1, 27, 1, 0), (3, 27, 1, 0),
             (2, 24, 0, 0), (2, 512, 0, 0), (2, 27, 1, 0), (0, 512, 0, 1), (1, 515, 1, 1), (3, 512, 0, 1))
    for encoding, enc_dim, progressive, want in cases:
        a.encoding, a.enc_dim, a.progressive = encoding, enc_dim, progressive
        assert lib.sininn_flownet_supported(C.byref(a)) == want, (encoding, enc_dim, progressive)
    a.encoding, a.enc_dim, a.progressive = 4, 24, 0
    assert lib.sininn_flownet_forward_workspace_bytes(C.byref(a)) == 0          # plain PE reads W1 [256][24] in place
    assert lib.sininn_flownet_encgrad_workspace_bytes(C.byref(a)) == 0
    g = (C.c_float * 768)()
    rc = lib.sininn_flownet_backward(C.byref(a), C.byref(_lib.FlowNetCall(mode=_lib.ENCGRAD, g_enc_a=C.cast(g, C.c_void_p))), None)      # refused on the encoding, before any launch
    assert rc != 0 and b'SININN_FLOWNET_FOURIER' in lib.sininn_last_error()
    a.T, a.H, a.W = 2, 8, 8
    assert lib.sininn_flownet_forward(C.byref(a), None, None) != 0                    # no pointers: refused before any launch
    assert b'null' in lib.sininn_last_error()
    a.hidden = 128
    assert lib.sininn_flownet_forward(C.byref(a), None, None) != 0
    assert b'PE' in lib.sininn_last_error()
    a.hidden, a.enc_dim, a.progressive = 256, 27, 1
    assert lib.sininn_flownet_forward_workspace_bytes(C.byref(a)) == 256 * (32 + 4) * 4
    assert flownet.positional_model_dict == {'PE': flownet.PEModel, 'PPE': flownet.PPEModel}
    assert flownet.ModelParams().num_frequencies_pe == 4
    for name in NETS:
        with pytest.raises(NotImplementedError):
            flownet.flow_fields(build(name), torch.tensor([0.0, 0.5]), 8, 8, 1.0)
    fake = torch.zeros(2)
    with pytest.raises(ValueError):
        flownet._args(build('PPE'), fake, fake, fake, 1.0)                      # a progressive network without a mask
    with pytest.raises(ValueError):
        flownet._args(flownet.PEModel(flownet.ModelParams(hidden_dim=128)), fake, fake, fake, 1.0)
    for nf in (3, 5):
        with pytest.raises(ValueError):
            flownet._args(flownet.PEModel(flownet.ModelParams(num_frequencies_pe=nf)), fake, fake, fake, 1.0)


@pytest.mark.parametrize('name', NETS)
def test_command_line_takes_the_positional_networks(name):
    from sin_inn_amd import flownet, progressive
    m = flow_main()
    assert m.OUT_OF_SCOPE_NETWORKS == ('siren', 'MPFF') and len(m.NETWORKS) == 12
    args = m.get_args(['train', '--net', name])
    assert args.net == name and name in m.NETWORKS
    net = m.build_net(args)
    assert args.net_name == name
    if name == 'PPE':
        assert isinstance(net, progressive.LinearControllerEarly) and isinstance(net.model, flownet.PPEModel)
        assert net.encoding_dim == 27 and net.block_size == 6 and net.block_iterations == 250
        short = m.get_args(['train', '--net', name, '--epochs', '3'])
        ctl = m.build_net(short)
        assert ctl.block_iterations == 1 and ctl.progress_iterations == 3
    else:
        assert isinstance(net, flownet.PEModel) and net.encoding_dim == 24


@pytest.mark.parametrize('name', NETS)
def test_state_dict_round_trip(name):
    from sin_inn_amd import flownet
    net = build(name)
    other = flownet.positional_model_dict[name](flownet.ModelParams())
    with torch.no_grad():
        for p in other.parameters():
            p.zero_()
        other.encode.freqs.zero_()
    other.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    for (ka, va), (kb, vb) in zip(net.state_dict().items(), other.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka


def test_state_dict_round_trip_of_a_wrapped_ppe():
    ctl = controller(build('PPE'))
    assert list(ctl.state_dict().keys()) == ['mask_stashed', 'model.encode.freqs'] + ['model.' + k for k in KEYS]
    for i in range(N_MID):
        ctl.stash_iteration(torch.tensor(0.5))
    torch.manual_seed(1)
    from sin_inn_amd import flownet
    other = controller(flownet.PPEModel(flownet.ModelParams()))
    other.load_state_dict({k: v.clone() for k, v in ctl.state_dict().items()})
    assert torch.equal(ctl.mask, other.mask) and other.mask.shape == (27,)
    for (ka, va), (kb, vb) in zip(ctl.state_dict().items(), other.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
