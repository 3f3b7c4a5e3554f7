"""CPU: the flow-field networks with learnable Fourier frequencies (RFFModel / PRFFModel of sin_inn_amd/flownet.py) against fixtures
written by the reference's own model.py and progressive_controller.py (tests/golden/make_golden_flownet_learnable.py), the float64
restatement that tests/test_gpu_flownet_learnable.py measures the kernels with, and the C ABI of the new backward entry point.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_refs import net_tensors, own_gates, restate  # noqa: E402

NETS = ('RFF', 'PRFF')
SEED = {'RFF': 707, 'PRFF': 808}
CASES = {'RFF': ('plain',), 'PRFF': ('ones', 'init', 'ramp')}
TIMES, GH, GW, SCALE, STRIDE = (0.0, 0.5), 20, 28, 3.0, 97
MAX_ITERATION, EPSILON, N_RAMP = 1000, 1e-3, 98
WKEYS = [f'model.model.{i}.{s}' for i in (0, 2, 4, 6) for s in ('weight', 'bias')]
PKEYS = ['encode.frequencies'] + WKEYS


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_learnable.npz'))


def build(name):
    from sin_inn_amd import flownet
    torch.manual_seed(SEED[name])
    return flownet.learnable_model_dict[name](flownet.ModelParams())


def f_eff(frequencies, magnitudes):
    """model.py:274: the matrix the network multiplies the poses with, in the dtype of `frequencies`"""
    return torch.nn.functional.normalize(frequencies, p=2, dim=0) * magnitudes.to(frequencies)[None, :]


def host_mask(gold, case):
    return None if case in ('plain', 'ones') else torch.from_numpy(gold[f'mask_{case}'])


@pytest.mark.parametrize('name', NETS)
def test_port_holds_the_reference_numbers(gold, name):
    net = build(name)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold[f'{name}_keys']]
    assert list(sd.keys())[:2] == ['encode.frequencies', 'encode.magnitudes']
    params = dict(net.named_parameters())
    assert list(params) == [str(k) for k in gold[f'{name}_pkeys']] == PKEYS       # encode.frequencies first
    for key, v in sd.items():
        if key in params:
            flat = v.detach().reshape(-1)
            assert np.array_equal(flat[:32].numpy(), gold[f'{name}_head_{key}']), key
            assert np.array_equal(flat[-32:].numpy(), gold[f'{name}_tail_{key}']), key
            assert flat.double().sum().item() == float(gold[f'{name}_sum_{key}']), key
        else:
            assert np.array_equal(v.numpy(), gold[f'{name}_buf_{key}']), key
    freq = net.encode.frequencies
    assert isinstance(freq, torch.nn.Parameter) and freq.requires_grad and tuple(freq.shape) == (3, 256)
    assert np.array_equal(freq.detach().numpy(), gold[f'{name}_frequencies'])
    assert float((freq.detach().double().norm(dim=0) - 1).abs().max()) < 1e-6            # unit-norm columns
    assert 'encode.magnitudes' in dict(net.named_buffers()) and tuple(net.encode.magnitudes.shape) == (256,)
    assert torch.equal(net.encode.effective_frequencies(), f_eff(freq, net.encode.magnitudes))
    prog = name == 'PRFF'
    assert net.is_progressive == prog and net.encoding_dim == (515 if prog else 512) and net.encode.output_channels == 512
    assert tuple(sd['model.model.0.weight'].shape) == (256, 515 if prog else 512)
    with pytest.raises(NotImplementedError):
        net(torch.zeros(4, 3))


def test_controller_masks_of_the_port(gold):
    """the port's controller around a PRFFModel gives the masks the fixture's cases were made under"""
    from sin_inn_amd import progressive
    ctl = progressive.LinearControllerEarly(build('PRFF'), MAX_ITERATION, epsilon=EPSILON)
    assert np.array_equal(ctl.mask.numpy(), gold['mask_init']) and float(ctl.mask.sum()) == 6.0
    for _ in range(N_RAMP):
        ctl.stash_iteration(torch.tensor(0.5))
    assert np.array_equal(ctl.mask.numpy(), gold['mask_ramp']) and ctl.mask[78:84].tolist() == [0.5] * 6
    assert list(ctl.state_dict().keys())[:3] == ['mask_stashed', 'model.encode.frequencies', 'model.encode.magnitudes']


@pytest.mark.parametrize('name', NETS)
def test_restatement_reproduces_the_reference_in_float64(gold, name):
    net = build(name)
    bufs, weights = net_tensors(net)
    freq, mag = bufs['encode.frequencies'], bufs['encode.magnitudes']
    times, ys, xs = torch.tensor(TIMES), torch.linspace(-1, 1, GH), torch.linspace(-1, 1, GW)
    up = torch.from_numpy(gold['up']).double()
    for case in CASES[name]:
        mask = host_mask(gold, case)
        f64 = freq.double().requires_grad_(True)
        w64 = [p.double().requires_grad_(True) for p in weights]
        flows = restate(name, f_eff(f64, mag), w64, times, ys, xs, SCALE, torch.float64, mask)
        ref = torch.from_numpy(gold[f'{name}_out64_{case}'])
        assert float((flows.detach() - ref).abs().max() / ref.abs().max()) < 1e-12, case
        with torch.no_grad():
            f32 = restate(name, f_eff(freq, mag), weights, times, ys, xs, SCALE, torch.float32, mask)
        ref32 = torch.from_numpy(gold[f'{name}_out32_{case}'])
        assert float((f32 - ref32).abs().max() / ref32.abs().max()) < 1e-4, case     # two fp32 evaluations (thread count, BLAS blocking)
        # forced gates equal to the ReLU's own decision change nothing
        gates = own_gates(name, f_eff(f64, mag), w64, times, ys, xs, mask)
        forced = restate(name, f_eff(f64, mag), w64, times, ys, xs, SCALE, torch.float64, mask, gates)
        assert float((forced.detach() - ref).abs().max() / ref.abs().max()) < 1e-12, case
        grads = torch.autograd.grad((forced * up).sum(), [f64] + w64)
        for key, g in zip(PKEYS, grads):
            flat = g.reshape(-1)
            sub = flat if flat.numel() <= 1024 else flat[::STRIDE]
            want = torch.from_numpy(gold[f'{name}_gsub_{case}_{key}'])
            assert float((sub - want).abs().max()) <= 1e-12 * float(want.abs().max()), (case, key)
            gabs = float(gold[f'{name}_gabs_{case}_{key}'])
            assert abs(flat.sum().item() - float(gold[f'{name}_gsum_{case}_{key}'])) <= 1e-12 * gabs, (case, key)
            assert abs(flat.abs().sum().item() - gabs) <= 1e-12 * gabs, (case, key)
        # the frequency gradient in full; normalize projects out its component along each column
        gf, want = grads[0], torch.from_numpy(gold[f'{name}_gfreq_{case}'])
        assert tuple(want.shape) == (3, 256) and float(want.abs().max()) > 0
        assert float((gf - want).abs().max()) <= 1e-12 * float(want.abs().max()), case
        along = (want * freq.double()).sum(0)
        assert float(along.abs().max()) <= 1e-6 * float(want.abs().max()), case      # fp32 columns are unit-norm to 1e-7
        if mask is not None:
            closed = (mask[3::2] == 0) & (mask[4::2] == 0)                            # sin and cos of a frequency both closed
            assert int(closed.sum()) > 0 and bool((want[:, closed] == 0).all()) and bool((want[:, ~closed] != 0).any(0).all()), case
    if name == 'PRFF':
        m = host_mask(gold, 'init')
        assert m[:6].tolist() == [1.0] * 6 and float(m.sum()) == 6.0                 # e2 = sin of frequency 1 is open, its cos is closed
        assert bool((torch.from_numpy(gold['PRFF_gfreq_init'])[:, :2] != 0).all())


def test_abi_and_refusals():
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, flownet
    lib = _lib.lib()
    assert lib.sininn_version() == 4
    header = open(os.path.join(ROOT, 'include', 'sininn.h')).read()
    for sym in ('sininn_flownet_encgrad_workspace_bytes', 'sininn_flownet_backward'):
        assert hasattr(lib, sym) and sym in _lib.EXPORTED and re.search(r'\b' + sym + r'\s*\(', header), sym
    for sym in ('sininn_flownet_backward_encgrad', 'sininn_flownet_backward_encgrad_spatial', 'sininn_flownet_backward_encgrad_points'):
        assert sym not in _lib.EXPORTED and not hasattr(lib, sym) and not re.search(r'\b' + sym + r'\s*\(', header), sym

    def backward_encgrad(a, g_enc_a, enc_workspace, enc_workspace_bytes, stream):
        """the ENCGRAD mode of sininn_flownet_backward, with the arguments the entry point of that name took"""
        call = _lib.FlowNetCall(mode=_lib.ENCGRAD, g_enc_a=g_enc_a and C.cast(g_enc_a, C.c_void_p),
                                enc_workspace=enc_workspace and C.cast(enc_workspace, C.c_void_p), enc_workspace_bytes=enc_workspace_bytes)
        return lib.sininn_flownet_backward(a, C.byref(call), stream)
    assert lib.sininn_sizeof(7) == C.sizeof(_lib.FlowNetArgs) == 280      # as before this entry point was added
    assert [f[0] for f in _lib.FlowNetArgs._fields_][-3:] == ['progressive', 'k_active', 'mask']
    a = _lib.FlowNetArgs()
    a.encoding, a.enc_dim, a.hidden, a.layers, a.out_dim = 1, 512, 256, 3, 4
    a.T, a.H, a.W = 2, 8, 8
    need = lib.sininn_flownet_encgrad_workspace_bytes(C.byref(a))
    assert need >= (512 * 256 + 3 * 256) * 4 and need % 16 == 0
    ws = (C.c_float * 4)()
    g = (C.c_float * 4)()
    # refused before any launch: nothing below is a device pointer and no GPU is needed
    a.encoding = 0
    assert lib.sininn_flownet_encgrad_workspace_bytes(C.byref(a)) == 0
    assert backward_encgrad(C.byref(a), g, ws, need, None) != 0
    assert b'encoding' in lib.sininn_last_error()
    a.encoding = 1
    assert backward_encgrad(C.byref(a), None, ws, need, None) != 0
    assert b'g_enc_a' in lib.sininn_last_error()
    assert backward_encgrad(C.byref(a), g, ws, need - 4, None) != 0
    assert b'enc_workspace' in lib.sininn_last_error()
    assert backward_encgrad(C.byref(a), g, None, need, None) != 0
    assert b'enc_workspace' in lib.sininn_last_error()
    a.struct_bytes = 8
    assert backward_encgrad(C.byref(a), g, ws, need, None) != 0
    assert b'struct_bytes' in lib.sininn_last_error()
    a.struct_bytes = C.sizeof(_lib.FlowNetArgs)
    assert backward_encgrad(C.byref(a), g, ws, need, None) != 0     # all of its own checks pass: the backward's null pointers
    assert b'flownet_backward' in lib.sininn_last_error()
    assert sorted(flownet.model_dict) == ['FFN', 'RBF', 'UFF']
    assert sorted(flownet.progressive_model_dict) == ['PFF', 'PRBF', 'PUFF']
    assert flownet.learnable_model_dict == {'RFF': flownet.RFFModel, 'PRFF': flownet.PRFFModel}
    net = build('RFF')
    with pytest.raises(NotImplementedError):
        flownet.flow_fields(net, torch.tensor([0.0, 0.5]), 8, 8, 1.0)
    with pytest.raises(NotImplementedError):
        flownet._args(net, torch.zeros(2), torch.zeros(2), torch.zeros(2), 1.0, enc_a=torch.zeros(3, 256))
