"""No GPU needed: the points mode of the flow networks (net(poses), sin_inn_amd.flownet.flow_at, the AT_POINTS mode of the call descriptor,
once the entry points sininn_*_points, whose names the refusals still carry) as far as the host decides it: the entry points and their ctypes
declarations, their refusals before any launch (null poses, n = 0, n = 2^22 + 1, a wrong
struct_bytes; each leaves a sentence that names the cause), an ABI that did not move (descriptor sizes, version 4), and the errors of
flow_at / net(poses) / controller(poses) on tensors no kernel can take.  The numbers are tests/test_gpu_flownet_points.py's.
"""
import ctypes as C
import os

import pytest
import torch

POINT_CALLS = ('sininn_flownet_forward_points', 'sininn_flownet_backward_points', 'sininn_flownet_backward_encgrad_points',
               'sininn_siren_forward_points', 'sininn_siren_backward_points')
AT_POINTS, ENCGRAD = 1, 4
# the five calls, by the names they had as entry points of their own: name -> (entry point, mode of the call descriptor)
ENTRY = {'sininn_flownet_forward_points': ('sininn_flownet_forward', AT_POINTS),
         'sininn_flownet_backward_points': ('sininn_flownet_backward', AT_POINTS),
         'sininn_flownet_backward_encgrad_points': ('sininn_flownet_backward', AT_POINTS | ENCGRAD),
         'sininn_siren_forward_points': ('sininn_siren_forward', AT_POINTS),
         'sininn_siren_backward_points': ('sininn_siren_backward', AT_POINTS)}
FAKE = 0x1000                                  # a non-null, 16-byte aligned address that is never read: every case is refused on the host


def flownet_args(_lib, encoding=0, enc_dim=512):
    a = _lib.FlowNetArgs()
    a.encoding, a.enc_dim, a.hidden, a.layers, a.out_dim, a.scale = encoding, enc_dim, 256, 3, 4, 1.0
    a.enc_a = a.enc_b = a.flows = a.dflows = a.saved = FAKE
    a.workspace = FAKE
    for l in range(4):
        a.w[l] = a.b[l] = a.gw[l] = a.gb[l] = FAKE
    a.saved_bytes = a.workspace_bytes = 1 << 40
    return a


def siren_args(_lib):
    a = _lib.SirenArgs()
    a.in_dim, a.hidden, a.layers, a.out_dim, a.omega, a.scale = 3, 256, 3, 4, 30.0, 1.0
    a.flows = a.dflows = a.saved = FAKE
    a.workspace = FAKE
    for l in range(5):
        a.w[l] = a.b[l] = a.gw[l] = a.gb[l] = FAKE
    a.saved_bytes = a.workspace_bytes = 1 << 40
    return a


def calls(_lib):
    """name -> (descriptor factory, lambda (args, poses, n) -> return code)"""
    lib = _lib.lib()

    def call(name):
        entry, mode = ENTRY[name]
        return lambda a, p, n: getattr(lib, entry)(C.byref(a), C.byref(_lib.FlowNetCall(
            mode=mode, poses=p, n=n, g_enc_a=FAKE, enc_workspace=FAKE, enc_workspace_bytes=1 << 40)), None)
    return {'sininn_flownet_forward_points': (lambda: flownet_args(_lib), call('sininn_flownet_forward_points')),
            'sininn_flownet_backward_points': (lambda: flownet_args(_lib), call('sininn_flownet_backward_points')),
            'sininn_flownet_backward_encgrad_points': (lambda: flownet_args(_lib, encoding=1), call('sininn_flownet_backward_encgrad_points')),
            'sininn_siren_forward_points': (lambda: siren_args(_lib), call('sininn_siren_forward_points')),
            'sininn_siren_backward_points': (lambda: siren_args(_lib), call('sininn_siren_backward_points'))}


def test_symbols_are_exported_and_declared():
    from sin_inn_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'sininn.h')).read()
    for name in sorted({entry for entry, _ in ENTRY.values()}):
        assert name in _lib.EXPORTED, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes[0] in (C.POINTER(_lib.FlowNetArgs), C.POINTER(_lib.SirenArgs))
        assert fn.argtypes[1] == C.POINTER(_lib.FlowNetCall) and fn.argtypes[-1] is C.c_void_p
    assert dict(_lib.FlowNetCall._fields_)['n'] is C.c_int64
    for name in POINT_CALLS:                       # the entry points these calls had are gone
        assert name not in _lib.EXPORTED and not hasattr(lib, name) and name + '(' not in header, name


def test_abi_did_not_move():
    from sin_inn_amd import _lib
    lib = _lib.lib()
    assert lib.sininn_version() == 4
    assert lib.sininn_sizeof(7) == C.sizeof(_lib.FlowNetArgs) == 280
    assert lib.sininn_sizeof(9) == C.sizeof(_lib.SirenArgs) == 280


@pytest.mark.parametrize('name', POINT_CALLS)
def test_refusals_before_any_launch(name):
    from sin_inn_amd import _lib
    lib = _lib.lib()
    make, call = calls(_lib)[name]
    # the sentence starts with the entry point (the encgrad call shares flownet_backward_points' checks past its own head)
    short = b'flownet_backward_points' if 'encgrad' in name else name[len('sininn_'):].encode()

    def refused(a, poses, n, *words):
        assert call(a, poses, n) != 0
        msg = lib.sininn_last_error()
        assert msg and (short in msg or name[len('sininn_'):].encode() in msg), msg
        for w in words:
            assert w in msg, (w, msg)

    refused(make(), None, 64, b'null poses')
    refused(make(), FAKE, 0, b'0 points')
    refused(make(), FAKE, (1 << 22) + 1, b'4194305 points', b'2^22')
    refused(make(), FAKE, -5, b'-5 points')
    a = make()
    a.struct_bytes -= 8
    refused(a, FAKE, 64, b'struct_bytes')
    # what the grid calls refuse is refused here too: a null weight, a short `saved`
    a = make()
    a.w[1] = None
    refused(a, FAKE, 64, b'null weight')
    if 'backward' in name:
        a = make()
        a.saved_bytes = 16
        refused(a, FAKE, 64, b'saved holds 16 bytes')
    # the descriptor's own grid is ignored: T = H = W = 0 and null axis vectors are what a points call is given (all of the above)
    a = make()
    assert (a.T, a.H, a.W) == (0, 0, 0) and not a.times and not a.ys and not a.xs


def test_grid_calls_still_refuse_their_own_way():
    """the shared points check kept the grid sentences"""
    from sin_inn_amd import _lib
    lib = _lib.lib()
    a = flownet_args(_lib)
    assert lib.sininn_flownet_forward(C.byref(a), None, None) != 0 and b'grid 0 x 0 x 0' in lib.sininn_last_error()
    a.T = a.H = a.W = 4
    assert lib.sininn_flownet_forward(C.byref(a), None, None) != 0 and b'null axis' in lib.sininn_last_error()
    s = siren_args(_lib)
    assert lib.sininn_siren_backward(C.byref(s), None, None) != 0 and b'grid 0 x 0 x 0' in lib.sininn_last_error()


def nets():
    from sin_inn_amd import flownet, progressive
    torch.manual_seed(3)
    opt = flownet.ModelParams()
    prbf = flownet.PRBFModel(opt)
    return {'RBF': flownet.RbfModel(opt), 'RFF': flownet.RFFModel(opt), 'siren': flownet.SirenModel(opt), 'PRBF': prbf,
            'early': progressive.LinearControllerEarly(flownet.PRBFModel(opt)), 'lin': progressive.LinearController(prbf)}


def test_flow_at_errors():
    from sin_inn_amd import flownet
    assert 'flow_at' in dir(flownet)
    for name, net in nets().items():
        with pytest.raises(NotImplementedError, match='GPU only'):
            flownet.flow_at(net, torch.zeros(4, 3))
        with pytest.raises(ValueError, match=r'\(\.\.\., 3\)'):
            flownet.flow_at(net, torch.zeros(4, 2))
        with pytest.raises(ValueError, match='fp32'):
            flownet.flow_at(net, torch.zeros(4, 3, dtype=torch.float64))
        with pytest.raises(NotImplementedError, match='no gradient with respect to the coordinates'):
            flownet.flow_at(net, torch.zeros(4, 3, requires_grad=True))


def test_calling_a_network_or_a_controller_on_cpu_poses_still_raises():
    for name, net in nets().items():
        with pytest.raises(NotImplementedError):
            net(torch.zeros(4, 3))
        with pytest.raises(NotImplementedError):
            net(torch.zeros(2, 5, 3))
    ctl = nets()['early']
    with pytest.raises(NotImplementedError):
        ctl(torch.zeros(4, 3), get_mask=True)
    with pytest.raises(NotImplementedError):
        ctl(torch.zeros(4, 3), override_mask=torch.ones(515))
    with pytest.raises(ValueError):
        ctl(torch.zeros(4, 2))


def test_low_level_wrappers_exist_and_refuse_cpu_poses():
    from sin_inn_amd import flownet
    net = nets()['RBF']
    for fn in ('flownet_forward_points', 'flownet_backward_points', 'siren_forward_points', 'siren_backward_points'):
        assert callable(getattr(flownet, fn)), fn
    with pytest.raises(NotImplementedError):
        flownet._args(net, torch.zeros(4, 3), None, None, 1.0)
