"""CPU: the spatially adaptive controller (sin_inn_amd.progressive.StashedSpatialController) against a fixture written by the reference's
own progressive_controller.py (tests/golden/make_golden_flownet_spatial.py): cells and weights of points (exact), blurred masks, the
incremental re-blur of the block in progress (exact against a full one), the state sequence through stash_iteration /
update_progress, state-dict keys and a save / load round trip; the float64 restatement with a per-point mask
(tests/flownet_spatial_refs.py) that tests/test_gpu_flownet_spatial.py measures the kernels with; and the C ABI: the descriptor
did not grow, the four spatial entry points exist and refuse bad calls before any launch.

The box blurs of the port are sums of slices, not conv3d: blurred masks are compared within 2e-6 absolute (values in [0, 1], 125
terms of at most 1/125 each: every partial sum is at most 1, rounded to 2^-24 relative, in either order).
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
from flownet_spatial_refs import cells, interp_mask, restate_points  # noqa: E402

CASES = {'PRBF': (404, 4), 'PFF': (505, 7)}
BLOCK_ITERATIONS, EPSILON = 8, 1e-3
BLUR_TOL = 2e-6
SD_KEYS = ('mask_stashed', 'in_progress', 'log_buffer', 'log_counter')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_spatial.npz'))


def build(name, device='cpu'):
    from sin_inn_amd import flownet, progressive
    seed, res = CASES[name]
    torch.manual_seed(seed)
    net = flownet.all_model_dict[name](flownet.ModelParams()).to(device)
    return progressive.StashedSpatialController(net, res, block_iterations=BLOCK_ITERATIONS, epsilon=EPSILON)


def rounds(ctl, pts, loss, n):
    for _ in range(n):
        ctl.interpolate(pts)                             # an evaluation: it leaves the stash
        ctl.stash_iteration(loss)


def advance(ctl, gold, name, upto):
    """the fixture's script up to a stage; returns the masks seen on the way"""
    pts, loss = torch.from_numpy(gold[f'{name}_stash_pts']), torch.from_numpy(gold[f'{name}_stash_loss'])
    seen = {'0': ctl.get_mask().clone()}
    for stage, n in (('3', 3), ('10', 7)):
        rounds(ctl, pts, loss, n)
        seen[stage] = ctl.get_mask().clone()
        if stage == upto:
            return seen
    ctl.update_progress()
    seen['p'] = ctl.get_mask().clone()
    if upto == 'p':
        return seen
    rounds(ctl, pts, loss, 3)
    seen['p3'] = ctl.get_mask().clone()
    return seen


@pytest.mark.parametrize('name', list(CASES))
def test_state_sequence_and_blurred_masks(gold, name):
    ctl = build(name)
    res = CASES[name][1]
    assert [ctl.res, ctl.k, ctl.block_size, ctl.block_iterations, ctl.progress_iterations] == gold[f'{name}_meta'].tolist()
    assert ctl.k == (5 if res ** 3 > 100 else 3) and ctl.name == 'stash_spatial' and ctl.is_progressive
    assert tuple(ctl.mask.shape) == (res ** 3, 515) and ctl.k_active == 12
    ctl.eval()                                           # update_mask puts it back in training mode and ramps all the same
    seen = advance(ctl, gold, name, 'p3')
    for stage, m in seen.items():
        want = gold[f'{name}_mask_{stage}']
        err = float(np.abs(m.numpy() - want).max())
        print(f'{name} blurred mask {stage}: max abs error {err:.3g}')
        assert err <= BLUR_TOL, (stage, err)
        assert np.array_equal(m.numpy() == 0, want == 0), stage
    assert ctl.training
    assert not np.array_equal(gold[f'{name}_mask_p'], gold[f'{name}_mask_p3'])
    assert bool((seen['p3'][:, ctl.k_active:] == 0).all()) and ctl.k_active == ctl.next_block == 18


@pytest.mark.parametrize('name', list(CASES))
def test_update_progress_state_dict_and_round_trip(gold, name):
    ctl = build(name)
    advance(ctl, gold, name, 'p')
    assert np.array_equal(ctl.in_progress.numpy(), gold[f'{name}_in_progress'])
    assert [ctl.cur_block, ctl.next_block] == gold[f'{name}_cur_next'].tolist() and ctl.iteration == 0
    sd = ctl.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold[f'{name}_keys']]
    assert tuple(sd.keys())[:4] == SD_KEYS
    for key in SD_KEYS:
        assert np.array_equal(sd[key].numpy(), gold[f'{name}_sd_{key}']), key
    other = build(name)
    other.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert torch.equal(other.mask, ctl.mask) and torch.equal(other.in_progress, ctl.in_progress)
    assert torch.equal(other.get_mask(), ctl.get_mask())
    assert other.k_active >= 12 and bool((other.get_mask()[:, other.k_active:] == 0).all())


@pytest.mark.parametrize('name', list(CASES))
def test_incremental_blur_equals_full_blur(gold, name):
    ctl = build(name)
    pts, loss = torch.from_numpy(gold[f'{name}_stash_pts']), torch.from_numpy(gold[f'{name}_stash_loss'])
    ctl.get_mask()
    for step in range(20):
        rounds(ctl, pts, loss, 1)
        if step % 8 == 7:
            ctl.update_progress()
        cached = ctl.get_mask()
        assert ctl._dirty is None
        assert torch.equal(cached, ctl.blur()), step     # six columns written in place == all 515 blurred afresh
    before = ctl.get_mask()
    rounds(ctl, pts, loss, 1)
    assert ctl.get_mask() is before                      # in place: the same tensor


@pytest.mark.parametrize('name', list(CASES))
def test_cells_interpolation_and_float64_restatement(gold, name):
    ctl = build(name)
    res = CASES[name][1]
    advance(ctl, gold, name, 'p3')
    pts = torch.from_numpy(gold[f'{name}_pts'])
    inds, alphas = ctl.cells(pts)
    assert np.array_equal(inds.numpy(), gold[f'{name}_inds']) and np.array_equal(alphas.numpy(), gold[f'{name}_alphas'])
    rinds, ralphas = cells(pts, res)                     # the helper the GPU tests use
    assert torch.equal(rinds, inds) and torch.equal(ralphas, alphas)
    assert float(alphas.sum(1).max()) > 1.5, 'no point within 1e-6 below a cell boundary: a0 + a1 = 2 is not covered'
    grid = torch.from_numpy(gold[f'{name}_mask_p3'])     # the reference's own grid: the blur is checked elsewhere
    interp = ctl.interpolate(pts)
    assert float((interp - torch.from_numpy(gold[f'{name}_interp'])).abs().max()) <= 8 * BLUR_TOL
    m64 = interp_mask(grid, res, pts)
    assert float((m64 - torch.from_numpy(gold[f'{name}_interp']).double()).abs().max()) <= 4e-6
    bufs, weights = net_tensors(ctl.model)
    out64 = restate_points(name, bufs, weights, pts, torch.float64, m64)
    want64, want32 = torch.from_numpy(gold[f'{name}_out64']), torch.from_numpy(gold[f'{name}_out32'])
    err = float((out64 - want64).abs().max() / want64.abs().max())
    unit = float((want32.double() - want64).abs().max() / want64.abs().max())
    print(f'{name}: float64 restatement vs fixture {err:.3g} (fp32 reference deviates {unit:.3g})')
    assert err <= 1e-10


def test_stash_needs_a_per_point_loss_and_three_dimensions(gold):
    from sin_inn_amd import flownet, progressive
    ctl = build('PRBF')
    ctl.interpolate(torch.from_numpy(gold['PRBF_stash_pts']))
    with pytest.raises(ValueError, match='per-point loss'):
        ctl.stash_iteration(torch.tensor(0.5))
    with pytest.raises(ValueError, match='mask_dim'):
        progressive.StashedSpatialController(ctl.model, 4, mask_dim=2)
    assert progressive.StashedSpatialController(ctl.model, 1).res == 3
    with pytest.raises(NotImplementedError):
        flownet.flow_fields(ctl, torch.tensor([0.0]), 4, 4, 1.0)     # the kernels run on the GPU only


def test_abi_unchanged_and_spatial_entry_points_refuse_before_any_launch():
    from sin_inn_amd import _lib
    h = _lib.lib()
    assert h.sininn_sizeof(7) == 280 and h.sininn_sizeof(10) == C.sizeof(_lib.FlowNetCall) and h.sininn_sizeof(11) == 0 and h.sininn_version() == 4
    cs = (C.c_float * 6)(0, 0, 0, 1, 1, 1)
    csp, fake = C.cast(cs, C.c_void_p), C.c_void_p(64)   # never dereferenced: every call below is refused first

    def args(encoding=0, enc_dim=515, progressive=1):
        a = _lib.FlowNetArgs()
        a.encoding, a.enc_dim, a.hidden, a.layers, a.out_dim, a.progressive = encoding, enc_dim, 256, 3, 4, progressive
        return a

    def spatial(entry, mode, *tail):
        """the SPATIAL mode of an entry point: lambda (args, grid, res, centre_scale) -> return code"""
        return lambda a, g, r, c: getattr(h, entry)(C.byref(a), C.byref(_lib.FlowNetCall(
            mode=_lib.SPATIAL | mode, grid=g, res=r, centre_scale=c, g_enc_a=fake, enc_workspace=fake, enc_workspace_bytes=1 << 30)), *tail, None)

    calls = {        # by the names the modes had as entry points of their own
        'sininn_flownet_forward_spatial': spatial('sininn_flownet_forward', 0),
        'sininn_flownet_backward_spatial': spatial('sininn_flownet_backward', 0),
        'sininn_flownet_backward_encgrad_spatial': spatial('sininn_flownet_backward', _lib.ENCGRAD),
        'sininn_flownet_sample_mask': spatial('sininn_flownet_sample_mask', 0, fake),
    }
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'sininn.h')).read()
    for name in ('sininn_flownet_forward', 'sininn_flownet_backward', 'sininn_flownet_sample_mask'):
        assert name in _lib.EXPORTED
    for name in ('sininn_flownet_forward_spatial', 'sininn_flownet_backward_spatial', 'sininn_flownet_backward_encgrad_spatial'):
        assert name not in _lib.EXPORTED and not hasattr(h, name) and name + '(' not in header, name
    for name, call in calls.items():
        enc = 1 if 'encgrad' in name else 0
        for why, needle, a, g, r in (('null grid', 'null grid', args(enc), None, 5),
                                     ('res < 3', 'at least 3', args(enc), fake, 2),
                                     ('32-bit indexing', '32-bit', args(enc), fake, 200),
                                     ('PPE', 'PPE', args(4, 27), fake, 5),
                                     ('not progressive', 'progressive', args(enc, 512, 0), fake, 5)):
            assert call(a, g, r, csp) != 0, (name, why)
            msg = h.sininn_last_error().decode()
            assert needle in msg, (name, why, msg)
    assert calls['sininn_flownet_forward_spatial'](args(), fake, 5, None) != 0 and 'centre_scale' in h.sininn_last_error().decode()
