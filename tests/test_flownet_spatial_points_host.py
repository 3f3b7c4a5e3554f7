"""No GPU needed: per-point masks at pose lists (the AT_POINTS | SPATIAL modes of sininn_flownet_forward / _backward / _sample_mask, once
entry points of their own, whose names the refusals still carry; StashedSpatialController.__call__) as far as the host decides them: the
five calls refuse null poses, n = 0, n = 2^22 + 1, a null grid, a
descriptor that is not progressive and PPE before any launch, each under its own name; `note_poses` attributes a per-point loss to the cells
`interpolate` finds; `mask_by` / `expand_by` are refused by name; CPU poses are still refused as GPU-only.  The numbers are
tests/test_gpu_flownet_spatial_points.py's.
"""
import ctypes as C
import os

import pytest
import torch

FAKE = 0x1000                                  # a non-null, 16-byte aligned address that is never read: every case is refused on the host
# the five calls, by the names they had as entry points of their own (and still refuse under): name -> (entry point, mode of the call descriptor)
AT_POINTS, SPATIAL, ENCGRAD, POSEGRAD = 1, 2, 4, 8
ENTRY = {'sininn_flownet_forward_spatial_points': ('sininn_flownet_forward', AT_POINTS | SPATIAL),
         'sininn_flownet_backward_spatial_points': ('sininn_flownet_backward', AT_POINTS | SPATIAL),
         'sininn_flownet_backward_encgrad_spatial_points': ('sininn_flownet_backward', AT_POINTS | SPATIAL | ENCGRAD),
         'sininn_flownet_backward_posegrad_spatial_points': ('sininn_flownet_backward', AT_POINTS | SPATIAL | POSEGRAD),
         'sininn_flownet_sample_mask_points': ('sininn_flownet_sample_mask', AT_POINTS | SPATIAL)}
CALLS = ('sininn_flownet_forward_spatial_points', 'sininn_flownet_backward_spatial_points', 'sininn_flownet_backward_encgrad_spatial_points',
         'sininn_flownet_backward_posegrad_spatial_points', 'sininn_flownet_sample_mask_points')


def args(_lib, encoding=0, enc_dim=515, progressive=1):
    a = _lib.FlowNetArgs()
    a.encoding, a.enc_dim, a.hidden, a.layers, a.out_dim, a.scale, a.progressive = encoding, enc_dim, 256, 3, 4, 1.0, progressive
    a.k_active = enc_dim
    a.enc_a = a.enc_b = a.flows = a.dflows = a.saved = FAKE
    a.workspace = FAKE
    for l in range(4):
        a.w[l] = a.b[l] = a.gw[l] = a.gb[l] = FAKE
    a.saved_bytes = a.workspace_bytes = 1 << 40
    return a


def caller(_lib, name, g_poses=FAKE):
    """lambda (args, grid, poses, n) -> return code, every other pointer non-null"""
    lib = _lib.lib()
    cs = (C.c_float * 6)(0, 0, 0, 1, 1, 1)
    entry, mode = ENTRY[name]
    tail = (FAKE,) if 'sample_mask' in name else ()

    def call(a, grid, poses, n):
        c = _lib.FlowNetCall(mode=mode, poses=poses, n=n, grid=grid, res=3, centre_scale=C.cast(cs, C.c_void_p), g_enc_a=FAKE,
                             enc_workspace=FAKE, enc_workspace_bytes=1 << 40, g_poses=g_poses, extra_workspace=FAKE,
                             extra_workspace_bytes=1 << 40)
        return getattr(lib, entry)(C.byref(a), C.byref(c), *tail, None)
    return call


def test_symbols_are_exported_and_declared():
    from sin_inn_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'sininn.h')).read()
    for name in ('sininn_flownet_forward', 'sininn_flownet_backward', 'sininn_flownet_sample_mask'):
        assert name in _lib.EXPORTED, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes[0] == C.POINTER(_lib.FlowNetArgs)
        assert fn.argtypes[1] == C.POINTER(_lib.FlowNetCall) and fn.argtypes[-1] is C.c_void_p
    fields = dict(_lib.FlowNetCall._fields_)
    assert fields['res'] is C.c_int and fields['n'] is C.c_int64
    for name in CALLS:                             # the entry points these calls had are gone
        assert name not in _lib.EXPORTED and not hasattr(lib, name) and name + '(' not in header, name
    assert lib.sininn_version() == 4 and lib.sininn_sizeof(7) == C.sizeof(_lib.FlowNetArgs) == 280


@pytest.mark.parametrize('name', CALLS)
def test_refusals_before_any_launch(name):
    from sin_inn_amd import _lib
    lib = _lib.lib()
    call = caller(_lib, name)
    own = name[len('sininn_'):].encode()
    fourier = 'encgrad' in name                    # the frequency gradient exists for the Fourier encoding

    def make(**kw):
        return args(_lib, **{**(dict(encoding=1) if fourier else {}), **kw})

    def refused(a, grid, poses, n, *words):
        assert call(a, grid, poses, n) != 0
        msg = lib.sininn_last_error()
        assert msg.startswith(own + b':'), (own, msg)
        for w in words:
            assert w in msg, (w, msg)

    refused(make(), FAKE, None, 64, b'null poses')
    refused(make(), FAKE, FAKE, 0, b'0 points')
    refused(make(), FAKE, FAKE, (1 << 22) + 1, b'4194305 points', b'2^22')
    refused(make(), None, FAKE, 64, b'null grid')
    refused(make(enc_dim=512, progressive=0), FAKE, FAKE, 64, b'progressive')
    refused(make(encoding=4, enc_dim=27), FAKE, FAKE, 64, b'PPE')
    a = make()
    a.struct_bytes -= 8
    refused(a, FAKE, FAKE, 64, b'struct_bytes')
    if 'sample_mask' not in name:                  # what the twins refuse further down: a null weight, a short `saved`
        a = make()
        a.w[1] = None
        refused(a, FAKE, FAKE, 64, b'null weight')
    if 'backward' in name:
        a = make()
        a.saved_bytes = 16
        refused(a, FAKE, FAKE, 64, b'saved holds 16 bytes')
    if 'posegrad' in name:
        a = make()
        assert caller(_lib, name, g_poses=None)(a, FAKE, FAKE, 64) != 0
        assert b'flownet_backward_posegrad_spatial_points: null g_poses' in lib.sininn_last_error()


def controller(res=3):
    from sin_inn_amd import flownet, progressive
    torch.manual_seed(5)
    return progressive.StashedSpatialController(flownet.PRBFModel(flownet.ModelParams()), res)


def test_note_poses_attributes_the_loss_like_interpolate():
    gen = torch.Generator().manual_seed(2)
    x = torch.rand(200, 3, generator=gen) * 2 - 1
    loss = torch.rand(200, generator=gen)
    a, b = controller(), controller()
    a.note_poses(x.view(10, 20, 3))                # any leading shape: the list is (N, 3)
    a.stash_iteration(loss)
    b.interpolate(x)
    b.stash_iteration(loss)
    assert a.iteration == b.iteration == 1 and bool((a.log_counter != 0).any())
    assert torch.equal(a.log_buffer, b.log_buffer) and torch.equal(a.log_counter, b.log_counter)
    # a grid noted afterwards replaces the list, and the other way round
    times, ys, xs = torch.tensor([0.0, 0.5]), torch.linspace(-1, 1, 4), torch.linspace(-1, 1, 5)
    a.note_grid(times, ys, xs)
    assert a._last_poses().shape == (40, 3)
    a.note_poses(x)
    assert a._last_poses().shape == (200, 3) and a.stash == (None, None)
    with pytest.raises(RuntimeError, match='before any evaluation'):
        controller().stash_iteration(loss)


def test_mask_by_and_expand_by_are_refused_by_name():
    ctl = controller()
    x = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match='mask_by'):
        ctl(x, mask_by=x)
    with pytest.raises(NotImplementedError, match='expand_by'):
        ctl(x, expand_by=lambda m, p: m)


def test_cpu_poses_are_still_refused_as_gpu_only():
    from sin_inn_amd import flownet, progressive
    ctl = controller()
    x = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match='GPU only'):
        ctl(x)
    with pytest.raises(NotImplementedError, match='GPU only'):
        ctl(x, get_mask=True)
    with pytest.raises(NotImplementedError, match='GPU only'):
        flownet.flow_at(ctl, x, pose_grad=True)
    lin = progressive.LinearController(flownet.PRBFModel(flownet.ModelParams()))
    with pytest.raises(NotImplementedError, match='GPU only'):
        lin(x, override_mask=torch.ones(27, 515))
    for fn in ('flownet_forward_spatial_points', 'flownet_backward_spatial_points', 'flownet_sample_mask_points'):
        assert callable(getattr(flownet, fn)), fn
    with pytest.raises(NotImplementedError, match='GPU only'):
        flownet.flownet_sample_mask_points(ctl.model, x, torch.ones(27, 515), 3)
