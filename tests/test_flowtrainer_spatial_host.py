"""Host: `--spatially-adaptive` of the flow path without a GPU -- the command line, the block length, the resume rule of a spatial
controller, the trainer's `on_after_backward` hook, the refusals of sininn_flow_error_stash, and the float64 reference of the stash
(tests/flowstash_refs.py) against a point-by-point loop and against `StashedSpatialController.cells`."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowstash_refs as S  # noqa: E402
from sin_inn_amd import _lib, flownet, flowtrainer, progressive  # noqa: E402
from sin_inn_amd.lightning import LightningDataModule, LightningModule, Trainer  # noqa: E402


def flow_main():
    spec = importlib.util.spec_from_file_location('flow_main', os.path.join(ROOT, 'video-interpolation', 'main.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the command line ----

@pytest.mark.parametrize('net', ['PRBF', 'PFF', 'PUFF', 'PRFF', 'PRBFG'])
def test_cli_takes_the_switch_with_a_515_wide_progressive_network(net):
    args = flow_main().get_args(['train', '--net', net, '--spatially-adaptive'])
    assert args.spatially_adaptive and args.net == net and args.operation == 'train'


@pytest.mark.parametrize('net', ['PPE', 'RBF', 'FFN', 'PE'])
def test_cli_refuses_the_switch_with_any_other_network(net, capsys):
    with pytest.raises(SystemExit) as e:
        flow_main().get_args(['train', '--net', net, '--spatially-adaptive'])
    assert e.value.code == 2
    assert 'out of scope' in capsys.readouterr().err


@pytest.mark.parametrize('epochs, want', [(3, 1), (1000, 8), (112, 1), (224, 2)])
def test_build_net_block_iterations(epochs, want):
    m = flow_main()
    args = m.get_args(['train', '--net', 'PRBF', '--spatially-adaptive', '--epochs', str(epochs)])
    net = m.build_net(args, res=3)
    assert isinstance(net, progressive.StashedSpatialController) and net.res == 3 and net.epsilon == 1e-3
    assert net.block_iterations == want == max(3 * epochs // (4 * 84), 1)
    linear = m.build_net(m.get_args(['train', '--net', 'PRBF', '--epochs', str(epochs)]))
    assert isinstance(linear, progressive.LinearControllerEarly) and linear.block_iterations == want   # the same span of steps
    assert net.progress_iterations == linear.progress_iterations


# ---- checkpoints ----

def _spatial_trainer(epochs=1000):
    m = flow_main()
    args = m.get_args(['train', '--net', 'PRBF', '--spatially-adaptive', '--epochs', str(epochs)])
    args.net = m.build_net(args, res=3)
    if next(args.net.parameters()).is_cuda:                                  # a machine with a GPU builds it there; this test is the host's
        args.net = args.net.cpu()
    return flowtrainer.FlowTrainer(args)


@pytest.mark.parametrize('top, step, cur, nxt, iteration', [(0.0, 0, 6, 12, 0), (6.0, 5, 6, 12, 5), (29.5, 21, 24, 30, 5),
                                                             (30.0, 16, 30, 36, 0), (509.0, 3, 504, 515, 3), (510.0, 8, 510, 515, 0),
                                                             (515.0, 9, 510, 515, 1)])
def test_resume_rule_of_a_spatial_controller(top, step, cur, nxt, iteration):
    """cur_block: the largest multiple of block_size (6) not above floor(max(mask_stashed)), at least block_size; next_block by the
    class's rule (the last block takes the remainder); iteration = global_step % block_iterations (8 for 1000 epochs)"""
    model = _spatial_trainer()
    net = model.net
    assert net.block_iterations == 8 and net.block_size == 6 and net.mask_stashed.numel() == 27
    with torch.no_grad():
        net.mask_stashed.copy_(torch.linspace(0.25, 1.0, 27) * top)           # element 0 is NOT the maximum: the last one is
    model.on_load_checkpoint({'global_step': step})
    assert (net.cur_block, net.next_block, net.iteration) == (cur, nxt, iteration)


def test_spatial_state_dict_round_trip_on_the_host():
    src = _spatial_trainer()
    net = src.net
    net.in_progress[5] = False
    net.increase_block()
    net.increase_block()
    net._set_block(0.5)                                                      # half way up the third block: 18 + 3 = 21 (cell 5: 6)
    net.log_buffer[3], net.log_counter[3] = 2.0, 4.0
    sd = src.state_dict()
    assert float(sd['net.mask_stashed'].max()) == 21.0 and float(sd['net.mask_stashed'][5]) == 6.0
    dst = _spatial_trainer()
    dst.load_state_dict(sd)
    dst.on_load_checkpoint({'global_step': 19})
    assert (dst.net.cur_block, dst.net.next_block, dst.net.iteration) == (18, 24, 3)
    assert torch.equal(dst.net.in_progress, net.in_progress) and not bool(dst.net.in_progress[5])
    assert float(dst.net.log_buffer[3]) == 2.0 and float(dst.net.log_counter[3]) == 4.0
    assert torch.equal(dst.net.mask[5], net.mask[5]) and float(dst.net.mask[0].sum()) == 21.0


# ---- the stand-in trainer's hook ----

class _Recording(torch.optim.SGD):
    def __init__(self, params, calls):
        super().__init__(params, lr=0.1)
        self.calls = calls

    def zero_grad(self, set_to_none=False):
        self.calls.append('zero_grad')
        super().zero_grad(set_to_none=set_to_none)

    def step(self, *a, **kw):
        self.calls.append('step')
        return super().step(*a, **kw)


class _Toy(LightningModule):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(3))
        self.automatic_optimization = True
        self.calls = []

    def training_step(self, batch, batch_idx):
        loss = ((self.w * batch[0]).sum() - 1) ** 2
        loss.register_hook(lambda g: self.calls.append('backward'))
        return loss

    def configure_optimizers(self):
        return _Recording(self.parameters(), self.calls)


class _Hooked(_Toy):
    def on_after_backward(self):
        assert self.w.grad is not None and bool(self.w.grad.abs().sum() > 0)  # the gradient of this step is there, not yet applied
        self.calls.append('after_backward')


class _Data(LightningDataModule):
    def train_dataloader(self):
        return [(torch.full((3,), float(i + 1)),) for i in range(3)]


def test_trainer_calls_on_after_backward_between_backward_and_step():
    model = _Hooked()
    Trainer(max_epochs=2, accelerator='cpu').fit(model, _Data())
    assert model.calls == ['zero_grad', 'backward', 'after_backward', 'step'] * 6
    plain = _Toy()                                                           # a module without the hook trains as before
    Trainer(max_epochs=2, accelerator='cpu').fit(plain, _Data())
    assert plain.calls == ['zero_grad', 'backward', 'step'] * 6
    assert torch.equal(plain.w.detach(), model.w.detach())


# ---- the C ABI refuses before it touches a device ----

def _abi_call(lib, **over):
    fake = C.c_void_p(4096)                                                  # never dereferenced: every refusal precedes the launches
    a = dict(s1=fake, i1=fake, m1=fake, s2=fake, i2=fake, m2=fake, cm=1, B=2, Cc=3, H=4, W=5, times=fake, ys=fake, xs=fake, res=3,
             buf=fake, cnt=fake, e=None, ws=fake, ws_floats=1 << 20)
    a.update(over)
    return lib.sininn_flow_error_stash(a['s1'], a['i1'], a['m1'], a['s2'], a['i2'], a['m2'], a['cm'], a['B'], a['Cc'], a['H'], a['W'],
                                       a['times'], a['ys'], a['xs'], a['res'], 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, a['buf'], a['cnt'], a['e'],
                                       a['ws'], a['ws_floats'], None)


@pytest.mark.parametrize('over, word', [(dict(s1=None), b'null pointer'), (dict(m2=None), b'null pointer'), (dict(xs=None), b'null pointer'),
                                        (dict(buf=None), b'null pointer'), (dict(cnt=None), b'null pointer'), (dict(ws=None), b'null pointer'),
                                        (dict(res=2), b'res must be'), (dict(res=1025), b'res must be'), (dict(cm=2), b'masks have 1 or 3'),
                                        (dict(Cc=1, cm=3), b'masks have 1 or 1'), (dict(Cc=2), b'1 or 3 channels'),
                                        (dict(B=0), b'bad extents'), (dict(W=-1), b'bad extents'), (dict(H=65536), b'at most 65535 rows'),
                                        (dict(ws_floats=10), b'workspace holds 10 floats'), (dict(buf=C.c_void_p(4098)), b'misaligned')])
def test_abi_refusals(over, word):
    lib = _lib.lib()
    assert _abi_call(lib, **over) != 0
    assert word in lib.sininn_last_error(), lib.sininn_last_error()


def test_abi_workspace_query():
    lib = _lib.lib()
    q = lib.sininn_flow_error_stash_workspace_floats
    assert q(3, 436, 1024, 50) == 3 * 436 * 50 + 3 * 2500 + 100              # R1 (one tile per row), R2, the two axis sums
    assert q(1, 5, 1031, 50) == 5 * 2 * 50 + 2500 + 100                      # a row of 1031 pixels takes two tiles
    assert q(1, 1, 1, 2) == 0 and q(0, 1, 1, 3) == 0 and q(1, 1, 1, 1025) == 0
    assert 'sininn_flow_error_stash' in _lib.EXPORTED and lib.sininn_version() == 4


def test_operator_refuses_cpu_tensors():
    z = torch.zeros(1, 3, 2, 2)
    with pytest.raises(NotImplementedError, match='GPU only'):
        flowtrainer.error_stash(z, z, z, z, z, z, torch.zeros(1), torch.zeros(2), torch.zeros(2), 3, (0, 0, 0, 1, 1, 1), torch.zeros(27),
                                torch.zeros(27))


# ---- the reference itself ----

def _loop_reference(e, times, ys, xs, res, cs):
    """point by point, corner by corner, in numpy scalars: fp32 for the cell arithmetic, float64 for the sums"""
    f = np.float32
    buf, cnt, n = np.zeros(res ** 3), np.zeros(res ** 3), np.zeros(res ** 3, dtype=np.int64)

    def axis(v, d):
        x = f(f(v) - f(cs[d])) * f(cs[3 + d])
        u = f(f(f(f(x + f(1)) / f(2)) * f(max(res - 2, 1))) + f(.5))
        lo, hi = np.floor(u), np.ceil(f(u + f(1e-6)))
        clamp = lambda i: int(min(max(i, 0), res - 1))
        return (clamp(lo), clamp(hi)), (f(hi - u), f(u - lo))

    for b, t in enumerate(times):
        for y, vy in enumerate(ys):
            for x, vx in enumerate(xs):
                (it, at), (iy, ay), (ix, ax) = axis(t, 0), axis(vy, 1), axis(vx, 2)
                for k in range(8):
                    st, sy, sx = (k >> 2) & 1, (k >> 1) & 1, k & 1
                    cell = it[st] + res * (iy[sy] + res * ix[sx])
                    alpha = f(f(at[st] * ay[sy]) * ax[sx])
                    buf[cell] += float(alpha) * e[b, y, x]
                    cnt[cell] += float(alpha)
                    n[cell] += 1
    return buf, cnt, n


@pytest.mark.parametrize('res, cs', [(3, (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)), (7, (0.5, 0.2, 0.5, 2.0, 2.0 / 2.2, 0.4)),
                                     (4, (0.0, 0.0, 0.0, 1.5, 1.0, 1.0))])   # the last one pushes times past the grid: the clamp
def test_reference_against_a_point_loop(res, cs):
    g = torch.Generator().manual_seed(res)
    e = torch.rand(2, 3, 5, generator=g, dtype=torch.float64)
    times = torch.tensor([0.0, 1.0]) if res == 7 else torch.tensor([-1.0, 1.0])
    ys = torch.linspace(-0.9, 1.3, 3) if res == 7 else torch.linspace(-1, 1, 3)
    xs = torch.linspace(-2, 3, 5) if res == 7 else torch.linspace(-1, 1, 5)
    buf, cnt, n = S.stash(e, times, ys, xs, res, cs)
    lbuf, lcnt, ln = _loop_reference(e.numpy(), times.numpy(), ys.numpy(), xs.numpy(), res, cs)
    assert np.array_equal(n.numpy(), ln) and int(n.sum()) == 8 * 30
    np.testing.assert_allclose(buf.numpy(), lbuf, rtol=1e-14, atol=0)
    np.testing.assert_allclose(cnt.numpy(), lcnt, rtol=1e-14, atol=0)


@pytest.mark.parametrize('scaled', [False, True])
def test_reference_cells_are_the_controllers(scaled):
    torch.manual_seed(0)
    net = progressive.StashedSpatialController(flownet.progressive_model_dict['PRBF'](flownet.ModelParams()), 5)
    times, ys, xs = torch.tensor([0.1, 0.9, 0.35]), torch.linspace(-0.8, 1.2, 7), torch.linspace(-2, 3, 11)
    gt, gh, gw = torch.meshgrid(times, ys, xs, indexing='ij')
    points = torch.stack((gt, gh, gw), dim=-1).view(-1, 3)
    if scaled:
        net.set_scale(points)
    else:
        times, ys, xs, points = times * 2 - 1, ys - 0.2, xs / 3, None         # inside [-1, 1]^3 as they are
        gt, gh, gw = torch.meshgrid(times, ys, xs, indexing='ij')
        points = torch.stack((gt, gh, gw), dim=-1).view(-1, 3)
    inds, alphas = net.cells(points)                                         # (N, 8): column k is corner k
    cells, weights = S.corners(times, ys, xs, 5, net.centre_scale_host())
    assert torch.equal(cells.reshape(8, -1).t(), inds) and torch.equal(weights.reshape(8, -1).t(), alphas)
    assert int(inds.min()) >= 0 and int(inds.max()) < 125


def test_error_map_is_the_integrand_of_the_l1_terms():
    g = torch.Generator().manual_seed(1)
    s1, i1, s2, i2 = (torch.rand(2, 3, 4, 6, generator=g) for _ in range(4))
    m1 = (torch.rand(2, 1, 4, 6, generator=g) > 0.3).float()
    m2 = (torch.rand(2, 3, 4, 6, generator=g) > 0.3).float()
    e = S.error_map(s1, i1, m1, s2, i2, m2)
    want = 0.5 * ((m1 * (s1 - i1)).abs().double().mean(1) + (m2 * (s2 - i2)).abs().double().mean(1))
    assert float((e - want).abs().max()) < 1e-7                               # fp32 differences on the right
    composed = flowtrainer.error_map(s1, i1, m1, s2, i2, m2)
    assert composed.dtype == torch.float32 and float(((composed - e) / e.clamp_min(1e-30)).abs().max()) < 8 * S.U
    assert bool((e[(m1.sum(1) + m2.sum(1)) == 0] == 0).all())
