"""CPU: the flow-field networks on two coordinates (ModelParams(domain_dim=2, std_rbf=50, std=50), the networks of
video-interpolation/pair_flow.py) against a fixture written by the reference's own model.py and progressive_controller.py
(tests/golden/make_golden_flownet_pair.py): keys, shapes and encoder buffers of the port bit for bit, the restatement of
tests/flownet_pair_refs.py (what tests/test_gpu_flownet_pair.py measures the kernels with) against the stored outputs, the 514-wide mask
and its controller, every refusal that remains at this dimension, and the library's support table per network and dimension.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_refs import net_tensors  # noqa: E402
from flownet_pair_refs import NETS, PARAMS, PROGRESSIVE, SEED, build, grid_poses, restate_at  # noqa: E402

MAX_ITERATION, EPSILON, N_RAMP, N_MID = 1000, 1e-3, 97, 100
ITERS = (1, 2, 3, 4, 5, 6, 97, 98, 100, 299, 300, 301, 500, 1000)
ENC_SHAPES = {'RBF': {'encode.centres': (512, 2), 'encode.sigma': (512,)}, 'FFN': {'encode.frequencies': (2, 256)},
              'UFF': {'encode.frequencies': (2, 256)}, 'RBFG': {'encode.offsets': (256, 2), 'encode.sigma': (256,)}}
PLAIN_OF = {'PRBF': 'RBF', 'PFF': 'FFN', 'PUFF': 'UFF', 'PRBFG': 'RBFG'}


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_pair.npz'))


def test_fixture_is_small_and_says_what_it_holds(gold):
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_pair.npz')) < 128 * 1024
    assert [str(n) for n in gold['names']] == list(NETS) and gold['seeds'].tolist() == [SEED[n] for n in NETS]
    assert gold['poses'].shape == (37, 2) and gold['poses'].dtype == np.float32
    assert not any('model.model' in k and ('_buf_' in k or '_head_' in k) for k in gold.files)   # no hidden-layer weights


@pytest.mark.parametrize('name', NETS)
def test_port_has_the_reference_keys_shapes_and_buffers(gold, name):
    net = build(name)
    sd = net.state_dict()
    prog = name in PROGRESSIVE
    assert list(sd.keys()) == [str(k) for k in gold[f'{name}_keys']]
    for (key, v), shape in zip(sd.items(), gold[f'{name}_shapes']):
        assert list(v.shape) == [int(d) for d in shape if d >= 0], key
    params = dict(net.named_parameters())
    bufs = [k for k in sd if k not in params]
    assert bufs and all(k.startswith('encode.') for k in bufs)
    for key in bufs:
        assert np.array_equal(sd[key].numpy(), gold[f'{name}_buf_{key}']), key
        assert tuple(sd[key].shape) == ENC_SHAPES[PLAIN_OF.get(name, name)][key]
    assert net.domain_dim == 2 and net.is_progressive == prog and net.encoding_dim == (514 if prog else 512)
    assert tuple(sd['model.model.0.weight'].shape) == (256, 514 if prog else 512) and tuple(sd['model.model.6.weight'].shape) == (4, 256)
    with pytest.raises(NotImplementedError):
        net(torch.zeros(4, 2))                                   # supported, and the kernels run on the GPU only


@pytest.mark.parametrize('name', NETS)
def test_restatement_reproduces_the_reference(gold, name):
    """float64: 1e-12; fp32: 1e-4, two fp32 evaluations (thread count, BLAS blocking): the tolerances of test_flownet_golden.py,
    test_flownet_progressive_golden.py and test_flownet_grid_golden.py for the same encodings"""
    bufs, weights = net_tensors(build(name))
    poses = torch.from_numpy(gold['poses'])
    cases = {'': None}
    if name in PROGRESSIVE:
        cases = {'': None, '_mid': torch.from_numpy(gold['mask_mid']), '_ramp': torch.from_numpy(gold['mask_ramp'])}
    with torch.no_grad():
        for tag, mask in cases.items():
            out = restate_at(name, bufs, weights, poses, 1.0, torch.float64, mask)
            ref = torch.from_numpy(gold[f'{name}_out64{tag}'])
            assert out.shape == (37, 4) and float((out - ref).abs().max() / ref.abs().max()) < 1e-12, tag
            if tag != '_ramp':
                out32 = restate_at(name, bufs, weights, poses, 1.0, torch.float32, mask)
                ref32 = torch.from_numpy(gold[f'{name}_out32{tag}'])
                assert float((out32 - ref32).abs().max() / ref32.abs().max()) < 1e-4, tag
        # the all-ones mask is the bare network
        if name in PROGRESSIVE:
            ones = restate_at(name, bufs, weights, poses, 1.0, torch.float64, torch.ones(514))
            assert torch.equal(ones, restate_at(name, bufs, weights, poses, 1.0, torch.float64, None))


def test_grid_poses_are_the_pair_script_s():
    p = grid_poses(3, 5)
    assert p.shape == (15, 2) and p[0].tolist() == [-1.0, -1.0] and p[4].tolist() == [-1.0, 1.0] and p[5].tolist() == [0.0, -1.0]
    assert torch.equal(p[:, 1].view(3, 5)[0], torch.linspace(-1, 1, 5)) and torch.equal(p[:, 0].view(3, 5)[:, 0], torch.linspace(-1, 1, 3))


def test_mask_is_514_wide_in_blocks_of_4_and_opens_as_the_reference_s(gold):
    from sin_inn_amd import progressive
    ctl = progressive.LinearControllerEarly(build('PRBF'), MAX_ITERATION, epsilon=EPSILON)
    assert ctl.encoding_dim == 514 and ctl.domain_dim == 2 and ctl.mask.shape == (514,)
    assert [ctl.block_size, ctl.block_iterations, ctl.progress_iterations] == gold['traj_meta'].tolist() == [4, 5, 635]
    assert np.array_equal(ctl.mask.numpy(), gold['mask_init']) and ctl.mask[:4].tolist() == [1.0] * 4 and float(ctl.mask.sum()) == 4.0
    at = 0
    for i in range(MAX_ITERATION):
        ctl.stash_iteration(torch.tensor(0.5 if i < 300 else 5e-4))
        if i + 1 in ITERS:
            assert np.array_equal(ctl.mask.numpy(), gold['traj_mask'][at]), i + 1
            assert ctl.cur_block == int(gold['traj_cur'][at]) and ctl.next_block == int(gold['traj_next'][at]), i + 1
            at += 1
    assert at == len(ITERS) and ctl.trigger
    ctl = progressive.LinearControllerEarly(build('PRBF'), MAX_ITERATION, epsilon=EPSILON)
    for i in range(N_MID):
        ctl.stash_iteration(torch.tensor(0.5))
        if i + 1 == N_RAMP:
            assert np.array_equal(ctl.mask.numpy(), gold['mask_ramp'])
            assert 0.0 < float(ctl.mask[ctl.cur_block]) < 1.0    # a block in progress: a fractional entry
    assert np.array_equal(ctl.mask.numpy(), gold['mask_mid'])
    from sin_inn_amd import flownet
    # call 100 has just opened a block whole (100 % 5 == 0): the next one is still shut
    assert flownet.last_open(ctl.mask) == ctl.cur_block == int(np.flatnonzero(gold['mask_mid'])[-1]) + 1 == 84


def params(**kw):
    from sin_inn_amd import flownet
    return flownet.ModelParams(**{**PARAMS, **kw})


@pytest.mark.parametrize('name,mode', [('RFF', 'RFF'), ('PRFF', 'RFF'), ('PE', 'PE'), ('PPE', 'PE'), ('MPFF', 'MPFF'), ('siren', 'SIREN')])
def test_networks_still_refused_at_two_coordinates(name, mode):
    from sin_inn_amd import flownet, progressive
    net = flownet.flow_model_dict[name](params())
    fake = torch.zeros(2)
    with pytest.raises(ValueError, match=f'domain_dim 2.*{mode}'):
        flownet.flow_fields(net, None, 8, 8, 1.0)
    with pytest.raises(ValueError, match=f'domain_dim 2.*{mode}'):
        flownet.flow_at(net, torch.zeros(4, 2))
    with pytest.raises(ValueError, match='domain_dim 2'):
        (flownet._siren_args if name == 'siren' else flownet._args)(net, None, fake, fake, 1.0)
    if net.is_progressive:
        with pytest.raises(ValueError, match=f'domain_dim 2.*{mode}'):
            flownet.flow_fields(progressive.LinearControllerEarly(net, 100, epsilon=1e-3), None, 8, 8, 1.0)


def test_modes_still_refused_at_two_coordinates():
    from sin_inn_amd import flownet, progressive
    net = build('PRBF')
    ctl = progressive.LinearControllerEarly(net, 100, epsilon=1e-3)
    with pytest.raises(ValueError, match='StashedSpatialController.*domain_dim == 3.*2'):
        progressive.StashedSpatialController(net, 5)
    for target in (net, ctl):
        with pytest.raises(ValueError, match='domain_dim 2.*override_mask grid'):
            flownet.flow_fields(target, None, 8, 8, 1.0, override_mask=torch.zeros(27, 514))
        with pytest.raises(ValueError, match='domain_dim 2.*pose_grad'):
            flownet.flow_at(target, torch.zeros(4, 2), pose_grad=True)
        with pytest.raises(ValueError, match='domain_dim 2.*times'):
            flownet.flow_fields(target, torch.zeros(1), 8, 8, 1.0)
        with pytest.raises(ValueError, match=r'domain_dim 2.*\(\.\.\., 2\)'):
            flownet.flow_at(target, torch.zeros(4, 3))
    with pytest.raises(ValueError, match='domain_dim 2.*override_mask grid'):
        ctl(torch.zeros(4, 2), override_mask=torch.zeros(27, 514))
    with pytest.raises(ValueError, match='domain_dim 2.*pose_grad'):
        net(torch.zeros(4, 2), pose_grad=True)
    fake = torch.zeros(2)
    with pytest.raises(ValueError, match='domain_dim 2.*per-point masks'):
        flownet._args(net, None, fake, fake, 1.0, spatial=True)
    with pytest.raises(ValueError, match='domain_dim 2.*times'):
        flownet._args(build('RBF'), fake, fake, fake, 1.0)
    # the other way round: a network on (t, y, x) called the two-coordinate way
    net3 = flownet.RbfModel(flownet.ModelParams())
    with pytest.raises(ValueError, match=r'domain_dim 3.*\(\.\.\., 3\)'):
        flownet.flow_at(net3, torch.zeros(4, 2))
    with pytest.raises(ValueError, match='domain_dim 3.*times'):
        flownet.flow_fields(net3, None, 8, 8, 1.0)
    with pytest.raises(ValueError, match='domain_dim 4'):
        flownet.flow_at(flownet.RbfModel(params(domain_dim=4)), torch.zeros(4, 4))
    # a supported network passes every refusal and stops at the device: the one that inverts with this feature
    with pytest.raises(NotImplementedError):
        flownet._args(build('RBF'), None, fake, fake, 1.0)
    with pytest.raises(NotImplementedError):
        flownet.flow_fields(build('RBF'), None, 8, 8, 1.0)


KINDS = {'RBF': 0, 'FFN': 1, 'UFF': 1, 'RBFG': 3, 'PE': 4, 'MPFF': 5}


def descriptor(kind, enc_dim, progressive):
    from sin_inn_amd import _lib
    a = _lib.FlowNetArgs()
    a.encoding, a.enc_dim, a.hidden, a.layers, a.out_dim, a.progressive = kind, enc_dim, 256, 3, 4, progressive
    return a


def test_library_support_table_per_network_and_dimension():
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'sininn.h')).read()
    for sym in ('sininn_flownet_supported_dim', 'sininn_flownet_forward', 'sininn_flownet_backward'):
        assert hasattr(lib, sym) and sym in _lib.EXPORTED and sym + '(' in header
    for sym in ('sininn_flownet_forward_dim', 'sininn_flownet_backward_dim', 'sininn_flownet_forward_points_dim',
                'sininn_flownet_backward_points_dim'):             # the dimension is a field of the call descriptor now
        assert not hasattr(lib, sym) and sym not in _lib.EXPORTED and sym + '(' not in header
    assert dict(_lib.FlowNetCall._fields_)['domain_dim'] is C.c_int

    def at(dim, **points):
        return C.byref(_lib.FlowNetCall(domain_dim=dim, **points))
    assert lib.sininn_version() == 4 and lib.sininn_sizeof(7) == C.sizeof(_lib.FlowNetArgs)      # additive: the descriptor is the one it was
    for name in ('RBF', 'FFN', 'UFF', 'RBFG'):
        for prog in (0, 1):
            two, three = descriptor(KINDS[name], 512 + 2 * prog, prog), descriptor(KINDS[name], 512 + 3 * prog, prog)
            assert lib.sininn_flownet_supported_dim(C.byref(two), 2) == 1, (name, prog)
            assert lib.sininn_flownet_supported_dim(C.byref(three), 3) == 1 and lib.sininn_flownet_supported(C.byref(three)) == 1
            if prog:
                assert lib.sininn_flownet_supported_dim(C.byref(two), 3) == 0 and lib.sininn_flownet_supported(C.byref(two)) == 0
                assert lib.sininn_flownet_supported_dim(C.byref(three), 2) == 0
                assert b'domain_dim 2' in lib.sininn_last_error() and b'514' in lib.sininn_last_error()
            assert lib.sininn_flownet_forward_workspace_bytes(C.byref(two)) == (256 * (512 + 4) * 4 if prog else 0)
    for kind, widths in ((KINDS['PE'], (16, 18, 24, 27)), (KINDS['MPFF'], (512, 514, 515))):
        for width in widths:
            for prog in (0, 1):
                assert lib.sininn_flownet_supported_dim(C.byref(descriptor(kind, width, prog)), 2) == 0
                assert b'domain_dim 2' in lib.sininn_last_error()
    a = descriptor(0, 512, 0)
    for dim in (0, 1, 4):
        assert lib.sininn_flownet_supported_dim(C.byref(a), dim) == 0 and f'domain_dim {dim}'.encode() in lib.sininn_last_error()
    a.struct_bytes -= 8
    assert lib.sininn_flownet_supported_dim(C.byref(a), 2) == 0
    # refused before any launch: T != 1 on the two-coordinate grid, a null mask
    a = descriptor(0, 514, 1)
    a.k_active, a.T, a.H, a.W = 514, 2, 8, 8
    assert lib.sininn_flownet_forward(C.byref(a), at(2), None) != 0 and b'mask' in lib.sininn_last_error()
    a = descriptor(0, 512, 0)
    a.T, a.H, a.W = 2, 8, 8
    assert lib.sininn_flownet_forward(C.byref(a), at(2), None) != 0 and b'T = 1' in lib.sininn_last_error()
    assert lib.sininn_flownet_backward(C.byref(a), at(2), None) != 0 and b'T = 1' in lib.sininn_last_error()
    assert lib.sininn_flownet_forward(C.byref(a), at(2, mode=_lib.AT_POINTS, poses=None, n=4), None) != 0 and b'poses' in lib.sininn_last_error()
    assert lib.sininn_flownet_forward(C.byref(a), at(5), None) != 0 and b'domain_dim 5' in lib.sininn_last_error()
