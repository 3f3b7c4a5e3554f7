"""GPU: the flow trainer under a spatially adaptive controller -- `flowtrainer.error_stash` (csrc/flowtrain.hip) on bare buffers against
the float64 reference of tests/flowstash_refs.py, then FlowTrainer under `build_net(args, res=7)` through the stand-in Trainer, a
checkpoint round trip, and `main.py train --spatially-adaptive` with the real res = 50.

Every bound is derived in tests/flowstash_refs.py from the roundings of the expressions (E: 6 U per element; a cell of the logs:
(n_terms + 12) U of the reference, n_terms the (point, corner) pairs of that cell); none is measured.  The masks are 0 / 1, as the
masks of a step are.  Each case is computed once (`runs`) and shared by the checks.
"""
import importlib.util
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowstash_refs as S  # noqa: E402
from sin_inn_amd import flowdata, flowloss, flowtrainer, progressive  # noqa: E402
from sin_inn_amd.lightning import Trainer  # noqa: E402

F64 = torch.float64


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def flow_main():
    spec = importlib.util.spec_from_file_location('flow_main', os.path.join(ROOT, 'video-interpolation', 'main.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _set_scale(times, ys, xs):
    """centre and scale as StashedSpatialController.set_scale makes them from the points of the grid, in fp32"""
    lo = torch.stack([v.min() for v in (times, ys, xs)])
    hi = torch.stack([v.max() for v in (times, ys, xs)])
    return tuple(float(v) for v in torch.cat(((hi + lo) / 2, 2 / (hi - lo))))


IDENTITY = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
# name: B, H, W, res, times, (ys range), (xs range), scaled as set_scale does
CASES = {
    'one_point': (1, 1, 1, 3, [-1.0], (-1, 1), (-1, 1), False),
    'odd_13x37': (3, 13, 37, 3, [-1.0, 0.0, 1.0], (-1, 1), (-1, 1), False),
    'scaled_24x40': (2, 24, 40, 7, [0.1, 0.9], (-0.8, 1.2), (-2, 3), True),
    'two_tiles_1031': (1, 5, 1031, 50, [0.3], (-1, 1), (-1, 1), False),
    'shared_time_cells_70x33': (4, 70, 33, 7, [-1.0, 0.1, 0.2, 1.0], (-1, 1), (-1, 1), False),   # 0.1 and 0.2: time cells 3 and 4 both
}


class _Cells(progressive.StashedSpatialController):
    """`cells` of the controller without its res^3 x 515 mask: what the composed form needs of it"""

    def __init__(self, res, centre_scale):
        torch.nn.Module.__init__(self)
        self.res, self.mask_dim = res, 3
        self.center_scale = torch.tensor(centre_scale, dtype=torch.float32).view(2, 1, 3)
        self.scale = self.scale_real


def _inputs(name, cm, dev):
    b, h, w, res, times, yr, xr, scaled = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + cm)
    s1, i1, s2, i2 = (torch.rand(b, 3, h, w, generator=g).to(dev) for _ in range(4))
    for s in (s1, s2):                                                       # splats with exact zeros: pixels nothing was splatted to
        s *= (torch.rand(b, 1, h, w, generator=g) > 0.15).to(dev)
    occl = [(torch.rand(b, 1, h, w, generator=g) > 0.3).float().to(dev) for _ in range(2)]   # masks with zeros
    if cm == 3:
        m1, m2 = flowtrainer.splat_mask(occl[0], s1), flowtrainer.splat_mask(occl[1], s2)    # (b, 3, h, w), as the step makes them
    else:
        m1, m2 = (o * (s != 0).all(1, keepdim=True) for o, s in zip(occl, (s1, s2)))
    if h > 2 and w > 2:
        m1[:, :, 1, 1] = 0                                                   # a pixel masked in every channel and both directions
        m2[:, :, 1, 1] = 0
    times = torch.tensor(times, device=dev)
    ys, xs = torch.linspace(*yr, h, device=dev), torch.linspace(*xr, w, device=dev)
    cs = _set_scale(times, ys, xs) if scaled else IDENTITY
    return (s1, i1, m1, s2, i2, m2), (times, ys, xs), res, cs


_RUNS = {}


@pytest.fixture(scope='module')
def runs(dev):
    def get(name, cm):
        if (name, cm) not in _RUNS:
            six, axes, res, cs = _inputs(name, cm, dev)
            e64 = S.error_map(*six)
            ref_buf, ref_cnt, n_terms = S.stash(e64, *axes, res, cs)
            zeros = lambda: torch.zeros(res ** 3, device=dev)
            buf, cnt, e = zeros(), zeros(), torch.full(e64.shape, float('nan'), device=dev)
            flowtrainer.error_stash(*six, *axes, res, cs, buf, cnt, error_out=e)
            once = (buf.clone(), cnt.clone())
            flowtrainer.error_stash(*six, *axes, res, cs, buf, cnt)
            again = (zeros(), zeros())
            flowtrainer.error_stash(*six, *axes, res, cs, *again)
            composed = (zeros(), zeros())
            ec = torch.empty_like(e)
            flowtrainer.error_stash_composed(*six, *axes, _Cells(res, cs).cells, *composed, error_out=ec)
            _RUNS[name, cm] = dict(six=six, axes=axes, res=res, cs=cs, e64=e64, ref=(ref_buf, ref_cnt), n_terms=n_terms, e=e, once=once,
                                   twice=(buf, cnt), again=again, composed=composed, e_composed=ec)
        return _RUNS[name, cm]
    return get


ALL = [(name, cm) for name in CASES for cm in (1, 3)]


@pytest.mark.parametrize('name, cm', ALL)
def test_error_map_against_float64(runs, name, cm):
    r = runs(name, cm)
    e, e64 = r['e'], r['e64']
    assert bool(torch.isfinite(e).all())                                     # every element was written
    err = (e.to(F64) - e64).abs()
    print(f'{name} cm={cm}: worst E error {float((err / e64.clamp_min(1e-300)).max()) / S.U:.2f} U of {S.E_ROUNDINGS}')
    assert bool((err <= S.E_ROUNDINGS * S.U * e64).all())
    m1, m2 = r['six'][2], r['six'][5]
    masked = (m1.sum(1) + m2.sum(1)) == 0
    assert name == 'one_point' or int(masked.sum()) > 0
    assert bool((e[masked] == 0).all())


@pytest.mark.parametrize('name, cm', ALL)
def test_logs_against_float64(runs, name, cm):
    r = runs(name, cm)
    assert int(r['n_terms'].sum()) == 8 * r['e64'].numel()
    S.check_logs(*r['once'], *r['ref'], r['n_terms'], what=f'{name} cm={cm}')


@pytest.mark.parametrize('name, cm', ALL)
def test_second_call_accumulates_and_calls_are_bitwise_equal(runs, name, cm):
    r = runs(name, cm)
    S.check_logs(*r['twice'], *r['ref'], r['n_terms'], calls=2, what=f'{name} cm={cm} twice')
    assert torch.equal(r['again'][0], r['once'][0]) and torch.equal(r['again'][1], r['once'][1])


@pytest.mark.parametrize('name, cm', ALL)
def test_fused_against_composed(runs, name, cm):
    """the composed form sums the same terms with index_add_, in some order: it has the budget of the fused form, the two differ by
    at most twice that"""
    r = runs(name, cm)
    S.check_logs(*r['composed'], *r['ref'], r['n_terms'], what=f'{name} cm={cm} composed')
    for got, other, ref in zip(r['once'], r['composed'], r['ref']):
        budget = 2 * (r['n_terms'].to(F64) + S.STASH_C) * S.U * ref
        assert bool(((got.to(F64) - other.to(F64)).abs() <= budget).all())
    e, ec, e64 = r['e'], r['e_composed'], r['e64']
    assert bool(((e.to(F64) - ec.to(F64)).abs() <= 2 * S.E_ROUNDINGS * S.U * e64).all())


@pytest.mark.parametrize('name, cm', [('scaled_24x40', 1), ('shared_time_cells_70x33', 3), ('two_tiles_1031', 3)])
def test_error_map_is_the_integrand_of_the_l1_kernels(runs, name, cm):
    """2 mean(E) = L1Loss(1)(S1, I1, m1) sum(m1) / numel(m1) + the same for direction 2.  L1Loss sums n = B C H W non-negative fp32 terms
    in an order of its own: n U of its value; the mask sums are counts below 2^24, exact; E carries its 6 U; the mean of E is taken in
    float64 here.  Products, the quotient and the sum of the two sides: 8 more."""
    r = runs(name, cm)
    s1, i1, m1, s2, i2, m2 = r['six']
    l1 = flowloss.L1Loss(1)
    want = sum(l1(s, i, m).to(F64) * m.sum().to(F64) / m.numel() for s, i, m in ((s1, i1, m1), (s2, i2, m2)))
    got = 2 * r['e'].to(F64).mean()
    tol = (s1.numel() + S.E_ROUNDINGS + 8) * S.U
    print(f'{name}: 2 mean(E) {float(got):.8f}, from L1Loss {float(want):.8f}, relative {abs(float(got / want) - 1):.2e} of {tol:.2e}')
    assert abs(float(got / want) - 1) <= tol


def test_operator_refuses_what_it_cannot_take(runs, dev):
    r = runs('odd_13x37', 1)
    buf, cnt = torch.zeros(27, device=dev), torch.zeros(27, device=dev)
    with pytest.raises(RuntimeError, match='res must be'):
        flowtrainer.error_stash(*r['six'], *r['axes'], 2, r['cs'], torch.zeros(8, device=dev), torch.zeros(8, device=dev))
    with pytest.raises(AssertionError, match='one time per frame'):
        flowtrainer.error_stash(*r['six'], r['axes'][0][:2], *r['axes'][1:], 3, r['cs'], buf, cnt)
    with pytest.raises(AssertionError, match='res\\^3'):
        flowtrainer.error_stash(*r['six'], *r['axes'], 3, r['cs'], buf[:26], cnt)
    with pytest.raises(AssertionError, match='fp32'):
        flowtrainer.error_stash(*r['six'], *r['axes'], 3, r['cs'], buf.double(), cnt)
    assert float(buf.abs().sum()) == 0 and float(cnt.abs().sum()) == 0       # a refused call wrote nothing


# ---- the trainer under the spatial controller ----

def _args(m, *extra):
    return m.get_args(['train', '--synthetic', '4', '24', '40', '--net', 'PRBF', '--spatially-adaptive', '--batch', '2', *extra])


class _Capturing(flowtrainer.FlowTrainer):
    """records, for every step, the tensors and the grid the stash used and the logs as update_progress found them"""

    def on_after_backward(self):
        stash, grid, net = self._stash, self.net._last_grid, self.net
        progress = net.update_progress

        def spy():
            self.captured.append(dict(stash=stash, grid=grid, buf=net.log_buffer.clone(), cnt=net.log_counter.clone()))
            progress()
        net.update_progress = spy
        try:
            super().on_after_backward()
        finally:
            del net.update_progress
        self.blocks.append(net.cur_block)


@pytest.fixture(scope='module')
def trained(dev, tmp_path_factory):
    m = flow_main()
    args = _args(m, '--epochs', '3')
    torch.manual_seed(0)
    args.net = m.build_net(args, res=7)
    model = _Capturing(args)
    model.captured, model.blocks = [], []
    video, _ = flowdata.get_video(args.input_video, args)
    trainer = Trainer(gpus=[0], max_epochs=3, check_val_every_n_epoch=4)
    trainer.fit(model, video)                                                # a "mask grid changed" error would surface here
    path = os.path.join(str(tmp_path_factory.mktemp('spatial')), 'last.ckpt')
    trainer.save_checkpoint(model, path)
    return m, model, video, path


def test_python_api_run(trained, dev):
    _, model, _, _ = trained
    net = model.net
    assert isinstance(net, progressive.StashedSpatialController) and net.res == 7 and net.block_iterations == 1
    assert next(net.parameters()).is_cuda and net.mask.is_cuda and net.log_buffer.is_cuda
    assert model.blocks == [12, 18, 24, 30, 36, 42]                          # update_progress ran after every step: one block of 6 each
    assert len(model.captured) == 6 and net.iteration == 0 and model._stash is None
    first = model.captured[0]
    buf, cnt = torch.zeros(343, device=dev), torch.zeros(343, device=dev)
    flowtrainer.error_stash(*first['stash'], *first['grid'], 7, net.centre_scale_host(), buf, cnt)
    assert torch.equal(buf, first['buf']) and torch.equal(cnt, first['cnt'])
    assert float(cnt.sum()) > 0 and float(buf.sum()) > 0
    ref_buf, ref_cnt, n_terms = S.stash(S.error_map(*first['stash']), *first['grid'], 7, net.centre_scale_host())
    S.check_logs(buf, cnt, ref_buf, ref_cnt, n_terms, what='step 1')


def test_stash_grid_refuses_a_pose_list_and_other_shapes(trained, dev):
    _, model, video, _ = trained
    net = model.net
    six = model.captured[0]['stash']
    wrong = tuple(t[:, :, :-1] for t in six)
    with pytest.raises(ValueError, match='the grid evaluated last'):
        net.stash_grid(*wrong)
    held = net._last_grid
    with torch.no_grad():
        net(torch.zeros(5, 3, device=dev))
    with pytest.raises(RuntimeError, match='pose list'):
        net.stash_grid(*six)
    net._last_grid, net._last_list = None, None
    with pytest.raises(RuntimeError, match='before any evaluation'):
        net.stash_grid(*six)
    net._last_grid = held
    assert net.iteration == 0                                                # no refused call counted as a step


def test_checkpoint_round_trip_reproduces_the_flows(trained, dev):
    m, model, video, path = trained
    args = _args(m, '--epochs', '3')
    args.net = m.build_net(args, res=7)
    back = flowtrainer.FlowTrainer.load_from_checkpoint(path, args=args).to(dev)
    assert back.net.cur_block == 42 and back.net.next_block == 48 and back.net.iteration == 0
    assert torch.equal(back.net.in_progress, model.net.in_progress) and torch.equal(back.net.mask, model.net.mask)
    model.net.eval(), back.net.eval()
    with torch.no_grad():
        for i in range(3):
            f1, _, t, s = video.testset[i][:4]
            a, b = (mod(f1.to(dev)[None], t.to(dev)[None], s) for mod in (model, back))
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), i


def test_command_line_run_at_res_50(dev, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    m = flow_main()
    common = ['--synthetic', '4', '24', '40', '--net', 'PRBF', '--spatially-adaptive', '--batch', '2', '--wandb', 'x', '--name', 's']
    m.main(['train', *common, '--epochs', '2'])
    ckpts = sorted(os.listdir(os.path.join('checkpoints', 'synthetic', 's')))
    assert ckpts == ['epoch=0.ckpt', 'epoch=1.ckpt']
    ck = torch.load(os.path.join('checkpoints', 'synthetic', 's', 'epoch=1.ckpt'), map_location='cpu')
    sd = ck['state_dict']
    assert sd['net.mask_stashed'].numel() == 50 ** 3 and sd['net.log_buffer'].numel() == 50 ** 3 and ck['global_step'] == 4
    # at res = 50 a batch of two frames visits two or three of the 50 time cells: the first update_progress opens the second block
    # around them and closes every cell whose blurred log is 0 -- the rest of the grid, the other frames' cells included -- at 6
    top = float(sd['net.mask_stashed'].max())
    assert 12.0 <= top <= 30.0 and top % 6 == 0 and float(sd['net.mask_stashed'].min()) == 6.0
    assert int(sd['net.in_progress'].sum()) < 50 ** 3
    m.main(['test', *common])
    out = capsys.readouterr().out
    assert out.count('test/EPE') == 2                                        # after training, and from `test`
    assert len([f for f in os.listdir('results') if f.startswith('flow_synthetic_s_epe_')]) >= 1
