"""CPU: the piecewise-linear progressive flow-field network MPFF (sin_inn_amd/flownet.py: MPFFModel, UniformPieceWiseEncoding) against a
fixture written by the reference's own model.py and progressive_controller.py (tests/golden/make_golden_flownet_piecewise.py), and the
float64 restatement of the encoding and the network that tests/test_gpu_flownet_piecewise.py measures the kernels with
(`encode_piecewise` of tests/flownet_piecewise_refs.py under `restate` of tests/flownet_refs.py).
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
import flownet_piecewise_refs as P  # noqa: E402
from flownet_piecewise_refs import GH, GW, KEYS, N_MID, N_RAMP, NAME, SCALE, STRIDE, TIMES, build, controller  # noqa: E402
from flownet_refs import net_tensors, own_gates, restate  # noqa: E402


@pytest.fixture(scope='module')
def gold():
    return P.gold()


def test_port_holds_the_reference_numbers(gold):
    net = build()
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold[f'{NAME}_keys']]
    assert list(sd.keys()) == ['encode.frequencies'] + KEYS
    params = dict(net.named_parameters())
    assert sorted(params) == sorted(KEYS)
    for key, v in sd.items():
        if key in params:
            flat = v.detach().reshape(-1)
            assert np.array_equal(flat[:32].numpy(), gold[f'{NAME}_head_{key}']), key
            assert np.array_equal(flat[-32:].numpy(), gold[f'{NAME}_tail_{key}']), key
            assert flat.double().sum().item() == float(gold[f'{NAME}_sum_{key}']), key
        else:
            assert np.array_equal(v.numpy(), gold[f'{NAME}_buf_{key}']), key
    assert net.encode.kind == 5 and net.encode.output_channels == 512 and net.domain_dim == 3
    assert net.is_progressive and net.encoding_dim == 515
    assert tuple(sd['model.model.0.weight'].shape) == (256, 515) and tuple(sd['model.model.6.weight'].shape) == (4, 256)
    freq, none = net.encode.kernel_buffers()
    assert none is None and tuple(freq.shape) == (3, 256) and freq.dtype == torch.float32
    norms = freq.norm(2, 0)
    assert bool((freq >= 0).all()) and bool((norms[1:] > norms[:-1]).all()) and 13.7 < float(norms[-1]) < 13.9
    with pytest.raises(NotImplementedError):
        net(torch.zeros(4, 3))


def test_the_gaussian_encoding_keeps_the_reference_draw_order():
    """model.py:660-667 restated inline: one randn (3, 256) times std / 2 pi, absolute values, columns sorted by norm; then the MLP draws"""
    from sin_inn_amd import flownet
    torch.manual_seed(5)
    enc = flownet.GaussianRandomPieceWiseEncoding(3, 256, 25)
    after = torch.rand(1)
    torch.manual_seed(5)
    f = (torch.randn(3, 256) * 25 / (2 * np.pi)).abs()
    f = f[:, f.norm(2, 0).argsort()]
    assert torch.equal(enc.frequencies, f) and torch.equal(after, torch.rand(1))
    assert enc.kind == 5 and enc.output_channels == 512 and isinstance(enc, flownet.PieceWiseEncoding)
    assert isinstance(build().encode, flownet.UniformPieceWiseEncoding)


def test_the_encoding_reproduces_the_reference_outside_the_domain(gold):
    """64 points of [-1.5, 1.5]^3 through the reference's own PieceWiseEncoding.forward in float64: u < 0 occurs, the values there lie in
    (-5, -1] as model.py:641-644 leaves them, and the restatement gives them to the last bit"""
    bufs, _ = net_tensors(build())
    poses = torch.from_numpy(gold['enc_poses'])
    want = torch.from_numpy(gold[f'{NAME}_enc64_out'])
    got = P.encode_piecewise(bufs, poses.double())
    assert torch.equal(got, want)
    u = P.piecewise_arg(bufs, poses.double())
    neg = (u < 0)[:, :, None].expand(-1, -1, 2).reshape(64, 512) & ((u[:, :, None] + torch.tensor([0.0, 1.0])) < 0).reshape(64, 512)
    assert int(neg.sum()) > 100 and float(want[neg].max()) <= -1.0 and float(want[neg].min()) > -5.0 and float(want[neg].min()) < -3.0
    assert float(want[~neg].min()) >= -1.0 and float(want[~neg].max()) <= 1.0


def test_restatement_reproduces_the_reference(gold):
    net = build()
    bufs, weights = net_tensors(net)
    times, ys, xs = torch.tensor(TIMES), torch.linspace(-1, 1, GH), torch.linspace(-1, 1, GW)
    w64 = [p.double().requires_grad_(True) for p in weights]
    masks = {k: torch.from_numpy(gold[f'mask_{k}']) for k in ('mid', 'ramp')}
    masks['ones'] = torch.ones(515)
    for k, mask in masks.items():
        flows = restate(NAME, bufs, w64, times, ys, xs, SCALE, torch.float64, mask)
        ref = torch.from_numpy(gold[f'{NAME}_out64_{k}'])
        assert float((flows.detach() - ref).abs().max() / ref.abs().max()) < 1e-12, k
        if k != 'ramp':
            with torch.no_grad():
                f32 = restate(NAME, bufs, weights, times, ys, xs, SCALE, torch.float32, mask)
            ref32 = torch.from_numpy(gold[f'{NAME}_out32_{k}'])
            assert float((f32 - ref32).abs().max() / ref32.abs().max()) < 1e-4, k      # two fp32 evaluations (thread count, BLAS blocking)
    mask = masks['ramp']
    forced = restate(NAME, bufs, w64, times, ys, xs, SCALE, torch.float64, mask, own_gates(NAME, bufs, w64, times, ys, xs, mask))
    ref = torch.from_numpy(gold[f'{NAME}_out64_ramp'])
    assert float((forced.detach() - ref).abs().max() / ref.abs().max()) < 1e-12
    grads = torch.autograd.grad((forced * torch.from_numpy(gold['up']).double()).sum(), w64)
    for key, g in zip(KEYS, grads):
        full = g
        g = g.reshape(-1)
        sub = g if g.numel() <= 1024 else g[::STRIDE]
        want = torch.from_numpy(gold[f'{NAME}_gsub_{key}'])
        assert float((sub - want).abs().max()) <= 1e-12 * float(want.abs().max()), key
        gabs = float(gold[f'{NAME}_gabs_{key}'])
        assert abs(g.sum().item() - float(gold[f'{NAME}_gsum_{key}'])) <= 1e-12 * gabs, key
        assert abs(g.abs().sum().item() - gabs) <= 1e-12 * gabs, key
        if key == 'model.model.0.weight':
            want = torch.from_numpy(gold[f'{NAME}_gcoord'])
            assert float((full[:, :3] - want).abs().max()) <= 1e-12 * float(want.abs().max())
            assert float(want.abs().max()) > 0 and bool((full[:, mask == 0] == 0).all())


def test_controller_wraps_mpff_unchanged(gold):
    ctl = controller(build())
    assert ctl.is_progressive and ctl.encoding_dim == 515 and ctl.domain_dim == 3 and ctl.block_size == 6
    assert list(ctl.state_dict().keys()) == ['mask_stashed', 'model.encode.frequencies'] + ['model.' + k for k in KEYS]
    for i in range(N_MID):
        ctl.stash_iteration(torch.tensor(0.5))
        if i + 1 == N_RAMP:
            assert np.array_equal(ctl.mask.numpy(), gold['mask_ramp'])
    assert np.array_equal(ctl.mask.numpy(), gold['mask_mid'])
    with pytest.raises(NotImplementedError):
        ctl(torch.zeros(4, 3))
    from sin_inn_amd import flownet, progressive
    torch.manual_seed(1)
    other = controller(flownet.MPFFModel(flownet.ModelParams()))
    other.load_state_dict({k: v.clone() for k, v in ctl.state_dict().items()})
    assert torch.equal(ctl.mask, other.mask) and other.mask.shape == (515,)
    for (ka, va), (kb, vb) in zip(ctl.state_dict().items(), other.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    spatial = progressive.StashedSpatialController(build(), 7)
    assert spatial.encoding_dim == 515 and tuple(spatial.mask.shape) == (343, 515)
    with pytest.raises(NotImplementedError):
        spatial(torch.zeros(4, 3))


def test_registry_and_the_closed_command_line():
    from sin_inn_amd import flownet
    assert flownet.PIECEWISE == 5
    assert flownet.piecewise_model_dict == {'MPFF': flownet.MPFFModel}
    assert 'MPFF' not in flownet.all_model_dict and len(flownet.all_model_dict) == 12
    assert flownet.flow_model_dict == {**flownet.all_model_dict, 'MPFF': flownet.MPFFModel, 'siren': flownet.SirenModel}
    assert flownet.MPFFModel.encoding == 'MPFF' and issubclass(flownet.MPFFModel, flownet.ProgressiveModel)
    assert isinstance(flownet.ENCODINGS['MPFF'](flownet.ModelParams()), flownet.UniformPieceWiseEncoding)
    spec = importlib.util.spec_from_file_location('flow_main_piecewise', os.path.join(ROOT, 'video-interpolation', 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.OUT_OF_SCOPE_NETWORKS == ('siren', 'MPFF') and 'MPFF' not in m.NETWORKS and len(m.NETWORKS) == 12


def test_abi_and_refusals():
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, flownet
    lib = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'sininn.h')).read()
    assert '#define SININN_FLOWNET_PIECEWISE 5' in header and '#define SININN_ABI_VERSION 4' in header
    assert lib.sininn_sizeof(7) == 280 == C.sizeof(_lib.FlowNetArgs) and lib.sininn_version() == 4
    a = _lib.FlowNetArgs()
    a.encoding, a.hidden, a.layers, a.out_dim = 5, 256, 3, 4
    for enc_dim, progressive, want in ((515, 1, 1), (512, 0, 0), (27, 1, 0), (515, 0, 0), (512, 1, 0)):
        a.enc_dim, a.progressive = enc_dim, progressive
        assert lib.sininn_flownet_supported(C.byref(a)) == want, (enc_dim, progressive)
        if not want:
            assert b'PieceWise progressive only: 515' in lib.sininn_last_error(), lib.sininn_last_error()
    a.enc_dim, a.progressive = 512, 0
    a.T, a.H, a.W = 2, 8, 8
    assert lib.sininn_flownet_forward(C.byref(a), None, None) != 0                  # the plain form: refused on the table, before any pointer
    assert b'unsupported network (encoding 5, 512' in lib.sininn_last_error() and b'PieceWise' in lib.sininn_last_error()
    a.encoding = 2                                                            # still no encoding of this library
    assert lib.sininn_flownet_supported(C.byref(a)) == 0
    a.encoding, a.enc_dim, a.progressive = 5, 515, 1
    assert lib.sininn_flownet_encgrad_workspace_bytes(C.byref(a)) == 0
    assert lib.sininn_flownet_forward_workspace_bytes(C.byref(a)) == 256 * (512 + 4) * 4
    a.encoding = 1
    fourier = lib.sininn_flownet_posegrad_workspace_bytes(C.byref(a), 0)
    a.encoding = 5
    assert lib.sininn_flownet_posegrad_workspace_bytes(C.byref(a), 0) == fourier > 0
    g = (C.c_float * 768)()
    rc = lib.sininn_flownet_backward(C.byref(a), C.byref(_lib.FlowNetCall(mode=_lib.ENCGRAD, g_enc_a=C.cast(g, C.c_void_p))), None)    # refused on the encoding, before any launch
    assert rc != 0 and b'SININN_FLOWNET_FOURIER' in lib.sininn_last_error()
    assert lib.sininn_flownet_forward(C.byref(a), None, None) != 0                  # no pointers: refused before any launch
    assert b'mask' in lib.sininn_last_error() or b'null' in lib.sininn_last_error()
    with pytest.raises(NotImplementedError):
        flownet.flow_fields(build(), torch.tensor([0.0, 0.5]), 8, 8, 1.0)
    with pytest.raises(NotImplementedError):
        flownet.flow_at(controller(build()), torch.zeros(4, 3))
    fake = torch.zeros(2)
    with pytest.raises(ValueError):
        flownet._args(build(), fake, fake, fake, 1.0)                         # a progressive network without a mask
    with pytest.raises(ValueError, match='PieceWise'):
        flownet._args(flownet.MPFFModel(flownet.ModelParams(hidden_dim=128)), fake, fake, fake, 1.0, mask=fake)


def test_composed_baseline_is_the_restatement():
    """tools/fit_flow.composed_piecewise (the tools' torch baseline) is model.py:638-644 as the restatement states it"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fit_flow
    from sin_inn_amd import flownet
    net = build()
    bufs, _ = net_tensors(net)
    poses = torch.rand(300, 3, generator=torch.Generator().manual_seed(2)) * 3 - 1.5
    assert fit_flow.PIECEWISE == flownet.PIECEWISE
    assert torch.equal(fit_flow.composed_piecewise(net.encode, poses), P.encode_piecewise(bufs, poses))
