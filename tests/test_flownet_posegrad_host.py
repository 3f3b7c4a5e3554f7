"""No GPU needed: the coordinate gradient of the flow networks (flow_at(.., pose_grad=True), the POSEGRAD mode of sininn_flownet_backward and
sininn_siren_backward, once entry points of their own, whose names the refusals still carry) as far as the host decides it: the symbols and
their declarations, the workspace size, the
refusals before any launch, each with a sentence under the entry point's name, and an ABI that did not move.  The numbers are
tests/test_gpu_flownet_posegrad.py's.
"""
import ctypes as C
import inspect
import os

import pytest
import torch

from test_flownet_points_host import FAKE, flownet_args, nets, siren_args

GONE = ('sininn_flownet_backward_posegrad_points', 'sininn_siren_backward_posegrad_points')   # the entry points the mode had
AT_POINTS, ENCGRAD, POSEGRAD = 1, 4, 8
ENCODINGS = {'RBF': (0, 512, 515), 'Fourier': (1, 512, 515), 'RBFG': (3, 512, 515), 'PE': (4, 24, 27)}


def test_symbols_are_exported_and_declared():
    from sin_inn_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'sininn.h')).read()
    for name in ('sininn_flownet_posegrad_workspace_bytes', 'sininn_flownet_backward', 'sininn_siren_backward'):
        assert name in _lib.EXPORTED, name
    assert lib.sininn_flownet_posegrad_workspace_bytes.restype is C.c_size_t
    for name, args in (('sininn_flownet_backward', _lib.FlowNetArgs), ('sininn_siren_backward', _lib.SirenArgs)):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes[0] is C.POINTER(args) and fn.argtypes[1] is C.POINTER(_lib.FlowNetCall)
        assert fn.argtypes[-1] is C.c_void_p
    assert dict(_lib.FlowNetCall._fields_)['n'] is C.c_int64
    for name in GONE:
        assert name not in _lib.EXPORTED and not hasattr(lib, name) and name + '(' not in header, name


def test_abi_did_not_move():
    from sin_inn_amd import _lib
    lib = _lib.lib()
    assert lib.sininn_version() == 4
    assert lib.sininn_sizeof(7) == C.sizeof(_lib.FlowNetArgs) == 280
    assert lib.sininn_sizeof(9) == C.sizeof(_lib.SirenArgs) == 280


@pytest.mark.parametrize('enc', list(ENCODINGS))
def test_workspace_size_is_non_zero_and_monotone(enc):
    """the packed W1 is at least one float per weight of the padded layer 1 (256 x the features) and the coordinate columns; asking for the
    frequency gradient as well never shrinks it, and adds exactly the encgrad call's own workspace; progressive or not, one size"""
    from sin_inn_amd import _lib
    lib = _lib.lib()
    kind, plain, prog = ENCODINGS[enc]
    sizes = []
    for width, progressive in ((plain, 0), (prog, 1)):
        a = flownet_args(_lib, encoding=kind, enc_dim=width)
        a.progressive = progressive
        without, with_enc = (lib.sininn_flownet_posegrad_workspace_bytes(C.byref(a), e) for e in (0, 1))
        assert without >= (plain + 3) * 256 * 4 and without % 16 == 0
        assert with_enc == without + lib.sininn_flownet_encgrad_workspace_bytes(C.byref(a)) >= without
        assert (with_enc > without) == (enc == 'Fourier')
        sizes.append(without)
    assert sizes[0] == sizes[1]
    a = flownet_args(_lib, encoding=2)
    assert lib.sininn_flownet_posegrad_workspace_bytes(C.byref(a), 0) == 0        # no encoding of this library
    assert lib.sininn_flownet_posegrad_workspace_bytes(None, 0) == 0


def test_flownet_refusals_before_any_launch():
    from sin_inn_amd import _lib
    lib = _lib.lib()
    name = b'flownet_backward_posegrad_points'

    def refused(a, poses, n, g_poses, g_enc, ws, nbytes, *words, who=name):
        c = _lib.FlowNetCall(mode=AT_POINTS | POSEGRAD | (ENCGRAD if g_enc else 0), poses=poses, n=n, g_poses=g_poses, g_enc_a=g_enc,
                             extra_workspace=ws, extra_workspace_bytes=nbytes)          # a non-null g_enc_a was how the old call said ENCGRAD
        assert lib.sininn_flownet_backward(C.byref(a), C.byref(c), None) != 0
        msg = lib.sininn_last_error()
        assert msg and who in msg, msg
        for w in words:
            assert w in msg, (w, msg)

    a = flownet_args(_lib)
    need = lib.sininn_flownet_posegrad_workspace_bytes(C.byref(a), 0)
    refused(a, FAKE, 64, None, None, FAKE, 1 << 40, b'null g_poses')
    refused(a, FAKE, 64, FAKE, None, None, 1 << 40, b'extra_workspace holds 0 bytes')
    refused(a, FAKE, 64, FAKE, None, FAKE, need - 4, b'extra_workspace holds', str(need).encode())
    refused(a, FAKE, 64, FAKE, None, FAKE + 4, 1 << 40, b'16-byte aligned')
    refused(a, FAKE, 64, FAKE, FAKE, FAKE, 1 << 40, b'SININN_FLOWNET_FOURIER')                 # RBF has no frequency gradient
    f = flownet_args(_lib, encoding=1)
    refused(f, FAKE, 64, FAKE, FAKE, FAKE, lib.sininn_flownet_posegrad_workspace_bytes(C.byref(f), 1) - 4, b'extra_workspace holds')
    b = flownet_args(_lib)
    b.struct_bytes -= 8
    refused(b, FAKE, 64, FAKE, None, FAKE, 1 << 40, b'struct_bytes')
    b = flownet_args(_lib, enc_dim=100)
    refused(b, FAKE, 64, FAKE, None, FAKE, 1 << 40, b'unsupported network')
    # everything the points calls refuse, under this entry point's name as well
    pts = name
    refused(a, None, 64, FAKE, None, FAKE, 1 << 40, b'null poses', who=pts)
    refused(a, FAKE, 0, FAKE, None, FAKE, 1 << 40, b'0 points', who=pts)
    refused(a, FAKE, (1 << 22) + 1, FAKE, None, FAKE, 1 << 40, b'4194305 points', who=pts)
    b = flownet_args(_lib)
    b.w[1] = None
    refused(b, FAKE, 64, FAKE, None, FAKE, 1 << 40, b'null weight', who=pts)
    b = flownet_args(_lib)
    b.saved_bytes = 16
    refused(b, FAKE, 64, FAKE, None, FAKE, 1 << 40, b'saved holds 16 bytes', who=pts)
    b = flownet_args(_lib)
    b.gw[2] = None
    refused(b, FAKE, 64, FAKE, None, FAKE, 1 << 40, b'null gradient pointer', who=pts)


def test_siren_refusals_before_any_launch():
    from sin_inn_amd import _lib
    lib = _lib.lib()

    def refused(a, poses, n, g_poses, *words):
        c = _lib.FlowNetCall(mode=AT_POINTS | POSEGRAD, poses=poses, n=n, g_poses=g_poses)
        assert lib.sininn_siren_backward(C.byref(a), C.byref(c), None) != 0
        msg = lib.sininn_last_error()
        assert msg and b'siren_backward_posegrad_points' in msg, msg
        for w in words:
            assert w in msg, (w, msg)

    refused(siren_args(_lib), FAKE, 64, None, b'null g_poses')
    refused(siren_args(_lib), None, 64, FAKE, b'null poses')
    refused(siren_args(_lib), FAKE, 0, FAKE, b'0 points')
    refused(siren_args(_lib), FAKE, (1 << 22) + 1, FAKE, b'4194305 points')
    a = siren_args(_lib)
    a.struct_bytes -= 8
    refused(a, FAKE, 64, FAKE, b'struct_bytes')
    a = siren_args(_lib)
    a.workspace_bytes = 16
    refused(a, FAKE, 64, FAKE, b'workspace holds 16 bytes')


def test_the_python_surface():
    from sin_inn_amd import flownet
    assert inspect.signature(flownet.flow_at).parameters['pose_grad'].default is False
    for fn in (flownet.flownet_backward_points, flownet.siren_backward_points):
        assert inspect.signature(fn).parameters['pose_grad'].default is False
    for name, net in nets().items():
        # without the keyword: as before; with it the call goes on, to the refusal of CPU poses
        with pytest.raises(NotImplementedError, match='no gradient with respect to the coordinates'):
            flownet.flow_at(net, torch.zeros(4, 3, requires_grad=True))
        with pytest.raises(NotImplementedError, match='GPU only'):
            flownet.flow_at(net, torch.zeros(4, 3, requires_grad=True), pose_grad=True)
        with pytest.raises(NotImplementedError, match='GPU only'):
            net(torch.zeros(4, 3, requires_grad=True), pose_grad=True)
