"""No GPU needed: the flow Jacobian as far as the host decides it.

  1. flow_jacobian_composed (the CPU path and the baseline of the fused call) against the float64 reference of tests/flownet_jacobian_refs.py
     under its budget rule, in fp32, for RBF, FFN and PRBF with k_active 3, 19, 515; the gates forced are the composed form's own.
  2. seeded defects of the composed form, each over the budget somewhere: a bias added to a tangent, a tangent gated by its own sign, the
     coordinate column dropped, the cosine feature's sign.
  3. the refusals of the Python surface, each a ValueError that names what is missing, and the keyword's grammar.
  4. the C refusals with fake pointers: every case is refused before any launch, under the entry point's own name; the ABI did not move.
  5. the trainer: with the network stubbed the step without the switches issues the calls it issued before, with them one extra flow_at;
     the command lines.
"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowgather_grad_refs as G  # noqa: E402
import flownet_jacobian_refs as J  # noqa: E402
from flownet_refs import net_tensors  # noqa: E402
from test_flownet_points_host import FAKE, flownet_args  # noqa: E402

F32, F64 = torch.float32, torch.float64
N = 96
SCALE = 3.0
AT_POINTS, SPATIAL, ENCGRAD, POSEGRAD = 1, 2, 4, 8


def build(name, k_active=None, seed=21):
    """(what flow_jacobian_composed takes, the model, override_mask or None, the restatement's name)"""
    from sin_inn_amd import flownet
    torch.manual_seed(seed)
    net = flownet.all_model_dict[name](flownet.ModelParams())
    mask = None
    if k_active is not None:
        mask = torch.zeros(net.encoding_dim)
        mask[:k_active] = 1.0
        if k_active > 4:
            mask[k_active - 2:k_active] = torch.tensor([0.75, 0.25])     # a block in progress
    return net, mask


def inputs(nd, seed=5):
    g = torch.Generator().manual_seed(seed)
    poses = torch.rand(N, 3, generator=g) * 2 - 1
    return poses, torch.randn(4, N, generator=g), torch.randn(nd, 4, N, generator=g)


def defective(net, mask, poses, dirs, gates, defect):
    """the composed form's tangent recursion restated here (planar outputs, scale SCALE) with one seeded error; `defect=None` is the sound
    recursion, which the test holds bitwise against the library's before it trusts the defective ones"""
    import math
    from sin_inn_amd import flownet
    lin = torch.nn.functional.linear
    e, de = flownet._encoding_with_tangents(net.encode, poses, dirs)
    if defect == 'cosine sign':
        de = [torch.cat((t[:, 0::2, None], -t[:, 1::2, None]), dim=2).reshape(t.shape) for t in de]
    if net.is_progressive:
        unit = torch.eye(3)
        e = torch.cat((poses, e), dim=1) * mask[None, :]
        de = [torch.cat(((0 * unit[d] if defect == 'coordinate column' else unit[d])[None, :].expand(poses.shape[0], 3), t), dim=1) * mask[None, :]
              for d, t in zip(dirs, de)]
    h, ts = e, de
    for l, layer in enumerate(net.linears()[:3]):
        g = gates[l].to(F32)
        h = lin(h, layer.weight, layer.bias) * g
        tpre = [lin(t, layer.weight, layer.bias if defect == 'bias in a tangent' else None) for t in ts]
        ts = [t * ((t > 0).to(F32) if defect == 'own sign' else g) for t in tpre]
    last = net.linears()[3]
    return (lin(h, last.weight, last.bias) * SCALE).t(), torch.stack([(lin(t, last.weight) * SCALE).t() for t in ts])


def composed(net, mask, poses, dirs, up, upj, gates=None, defect=None, restated=False):
    from sin_inn_amd import flownet
    params = [p for lin in net.linears() for p in (lin.weight, lin.bias)]
    for p in params:
        p.grad = None
    if restated or defect is not None:
        flow, jac = defective(net, mask, poses, dirs, gates, defect)
    else:
        flow, jac = flownet.flow_jacobian_composed(net, poses, SCALE, ''.join('tyx'[d] for d in dirs), override_mask=mask, planar=True, gates=gates)
    ((flow * up).sum() + (jac * upj).sum()).backward()
    return flow.detach(), jac.detach(), [p.grad.clone() for p in params]


def own_gates(net, mask, poses):
    """the ReLU decisions of the fp32 value pass of the composed form"""
    from sin_inn_amd import flownet
    with torch.no_grad():
        model, m = flownet._resolve_mask(net, mask, poses.device)
        e, _ = flownet._encoding_with_tangents(model.encode, poses, ())
        h = torch.cat((poses, e), 1) * m.tensor[None] if model.is_progressive else e
        gates = []
        for lin in model.linears()[:3]:
            h = torch.relu(torch.nn.functional.linear(h, lin.weight, lin.bias))
            gates.append(h > 0)
    return gates


CASES = [('RBF', None, (1, 2)), ('FFN', None, (0, 1, 2)), ('RBF', None, (0,)), ('PRBF', 3, (1, 2)), ('PRBF', 19, (0, 1, 2)), ('PRBF', 515, (1, 2))]


@pytest.mark.parametrize('name,k_active,dirs', CASES)
def test_composed_against_float64(name, k_active, dirs):
    net, mask = build(name, k_active)
    poses, up, upj = inputs(len(dirs))
    gates = own_gates(net, mask, poses)
    bufs, weights = net_tensors(net)
    ref = J.reference(name, bufs, weights, poses, SCALE, dirs, up, upj, mask, gates)
    flow, jac, grads = composed(net, mask, poses, dirs, up, upj, gates)
    assert tuple(jac.shape) == (len(dirs), 4, N) and bool((jac != 0).any())
    J.check_all(f'composed {name} k={k_active} {dirs}', dirs, flow, jac, grads, ref)
    # free gates are the forced ones: the decisions are the value pass's own
    flow2, jac2, grads2 = composed(net, mask, poses, dirs, up, upj)
    assert torch.equal(flow, flow2) and torch.equal(jac, jac2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    # float64 poses: the same function in float64, the reference's value to rounding
    from sin_inn_amd import flownet
    with torch.no_grad():
        _, jac64 = flownet.flow_jacobian_composed(net, poses.to(F64), SCALE, ''.join('tyx'[d] for d in dirs), override_mask=mask, planar=True,
                                                  gates=gates)
    assert jac64.dtype == F64 and J.relmax(jac64, ref[F64][1]) < 1e-10


@pytest.mark.parametrize('defect,name,k_active', [('bias in a tangent', 'RBF', None), ('own sign', 'RBF', None), ('own sign', 'FFN', None),
                                                  ('coordinate column', 'PRBF', 19), ('cosine sign', 'FFN', None)])
def test_a_seeded_defect_exceeds_the_budget(defect, name, k_active):
    dirs = (1, 2)
    net, mask = build(name, k_active)
    poses, up, upj = inputs(len(dirs))
    gates = own_gates(net, mask, poses)
    bufs, weights = net_tensors(net)
    ref = J.reference(name, bufs, weights, poses, SCALE, dirs, up, upj, mask, gates)
    flow, jac, grads = composed(net, mask, poses, dirs, up, upj, gates)
    assert not J.exceeds(dirs, jac, grads, ref)
    again = composed(net, mask, poses, dirs, up, upj, gates, restated=True)          # the restated recursion without a defect is the library's
    assert torch.equal(again[0], flow) and torch.equal(again[1], jac) and all(torch.equal(a, b) for a, b in zip(again[2], grads))
    _, jac, grads = composed(net, mask, poses, dirs, up, upj, gates, defect=defect)
    assert J.exceeds(dirs, jac, grads, ref), defect


def test_shapes_and_layouts():
    from sin_inn_amd import flownet
    net, _ = build('RBF')
    poses = inputs(1)[0]
    flow, jac = flownet.flow_jacobian_composed(net, poses.view(8, 12, 3), SCALE, 'xt')
    assert tuple(flow.shape) == (8, 12, 4) and tuple(jac.shape) == (8, 12, 4, 2)
    fp, jp = flownet.flow_jacobian_composed(net, poses, SCALE, 'tx', planar=True)                 # always in t, y, x order
    assert torch.equal(jp.permute(2, 1, 0).reshape(8, 12, 4, 2), jac) and torch.equal(fp.t().reshape(8, 12, 4), flow)
    assert flownet.jacobian_dirs(True) == (1, 2) and flownet.jacobian_dirs('xyt') == (0, 1, 2) and flownet.jacobian_dirs('t') == (0,)
    for bad in ('', 'yy', 'yz', 3, None, False):
        with pytest.raises(ValueError, match='jacobian'):
            flownet.jacobian_dirs(bad)


def test_python_refusals():
    from sin_inn_amd import flownet, progressive
    torch.manual_seed(1)
    opt = flownet.ModelParams()
    poses = torch.zeros(4, 3)
    refused = {'RFF': 'second derivative', 'PRFF': 'second derivative', 'RBFG': 'RBFG', 'PRBFG': 'RBFG', 'PE': 'PE / PPE', 'PPE': 'PE / PPE',
               'MPFF': 'MPFF', 'siren': 'SIREN'}
    for name, words in refused.items():
        net = flownet.flow_model_dict[name](opt)
        for call in (lambda: flownet.flow_at(net, poses, jacobian='yx'), lambda: flownet.flow_jacobian_composed(net, poses, 1.0, 'yx'),
                     lambda: net(poses, jacobian=True)):
            with pytest.raises(ValueError, match=words):
                call()
    pair = flownet.RbfModel(flownet.ModelParams(domain_dim=2))
    with pytest.raises(ValueError, match='domain_dim 2'):
        flownet.flow_at(pair, torch.zeros(4, 2), jacobian='yx')
    prbf = flownet.PRBFModel(opt)
    with pytest.raises(ValueError, match='per-point'):
        flownet.flow_at(progressive.StashedSpatialController(prbf, 4), poses, jacobian='yx')
    with pytest.raises(ValueError, match='per-point'):
        flownet.flow_at(progressive.LinearController(prbf), poses, override_mask=torch.ones(27, 515), jacobian='yx')
    rbf = flownet.RbfModel(opt)
    with pytest.raises(ValueError, match='pose_grad'):
        flownet.flow_at(rbf, poses, jacobian='yx', pose_grad=True)
    with pytest.raises(ValueError, match='no gradient to the poses'):
        flownet.flow_at(rbf, poses.clone().requires_grad_(True), jacobian='yx')
    with pytest.raises(ValueError, match='get_mask'):
        flownet.flow_at(prbf, poses, jacobian='yx', get_mask=True)
    with pytest.raises(ValueError, match='distinct letters'):
        flownet.flow_at(rbf, poses, jacobian='yy')
    with pytest.raises(NotImplementedError, match='GPU only'):                                  # a supported call on the CPU: flow_at's own refusal
        flownet.flow_at(rbf, poses, jacobian='yx')
    with pytest.raises(NotImplementedError, match='GPU only'):                                  # without the keyword: as before
        flownet.flow_at(rbf, poses)


def test_c_refusals_before_any_launch():
    from sin_inn_amd import _lib
    lib = _lib.lib()
    assert lib.sininn_version() == 4 and lib.sininn_sizeof(11) == 0
    assert lib.sininn_sizeof(7) == C.sizeof(_lib.FlowNetArgs) == 280 and lib.sininn_sizeof(10) == C.sizeof(_lib.FlowNetCall)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'sininn.h')).read()
    for name in ('sininn_flownet_jacobian_saved_bytes', 'sininn_flownet_jacobian_workspace_bytes', 'sininn_flownet_jacobian_forward',
                 'sininn_flownet_jacobian_backward'):
        assert name in _lib.EXPORTED and name + '(' in header, name
    n = 100
    a = flownet_args(_lib)
    saved = lib.sininn_flownet_saved_bytes(n)
    assert [lib.sininn_flownet_jacobian_saved_bytes(n, k) for k in (0, 1, 2, 3, 4)] == [0, saved, 2 * saved, 3 * saved, 0]
    need = lib.sininn_flownet_jacobian_workspace_bytes(C.byref(a), n, 2)
    assert need >= saved + (256 * 515 + 2 * 256 * 256 + 4 * 256) * 4 and need % 16 == 0
    assert lib.sininn_flownet_jacobian_workspace_bytes(None, n, 2) == 0 and lib.sininn_flownet_jacobian_workspace_bytes(C.byref(a), 0, 2) == 0
    BIG = 1 << 40

    def fwd(a, c, dirs=6, jac=FAKE, ts=FAKE, nbytes=BIG):
        return lib.sininn_flownet_jacobian_forward(C.byref(a), C.byref(c) if c is not None else None, dirs, jac, ts, nbytes, None)

    def bwd(a, c, dirs=6, djac=FAKE, ts=FAKE, nbytes=BIG, ws=FAKE, wsbytes=BIG):
        return lib.sininn_flownet_jacobian_backward(C.byref(a), C.byref(c) if c is not None else None, dirs, djac, ts, nbytes, ws, wsbytes, None)

    def call(mode=AT_POINTS, **kw):
        return _lib.FlowNetCall(mode=mode, poses=FAKE, n=n, **kw)

    def refused(rc, who, *words):
        assert rc != 0
        msg = lib.sininn_last_error()
        assert msg and who in msg, msg
        for w in words:
            assert w in msg, (w, msg)

    for run, who in ((fwd, b'flownet_jacobian_forward'), (bwd, b'flownet_jacobian_backward')):
        refused(run(a, call(), dirs=0), who, b'dirs')
        refused(run(a, call(), dirs=8), who, b'dirs')
        refused(run(a, None), who, b'null call descriptor')
        refused(run(a, call(mode=0)), who, b'AT_POINTS')
        refused(run(a, call(mode=AT_POINTS | SPATIAL)), who, b'SPATIAL')
        refused(run(a, call(mode=AT_POINTS | ENCGRAD)), who, b'ENCGRAD')
        refused(run(a, call(mode=AT_POINTS | POSEGRAD)), who, b'POSEGRAD')
        refused(run(a, call(mode=AT_POINTS | 0x10)), who, b'unknown mode bits 0x10')
        refused(run(a, call(domain_dim=2)), who, b'domain_dim 2')
        c = call()
        c.struct_bytes -= 8
        refused(run(a, c), who, b'struct_bytes')
        for enc, width in ((3, 512), (4, 24)):
            refused(run(flownet_args(_lib, encoding=enc, enc_dim=width), call()), who, b'SININN_FLOWNET_RBF')
        prog = flownet_args(_lib, encoding=5, enc_dim=515)
        prog.progressive = 1
        refused(run(prog, call()), who, b'SININN_FLOWNET_RBF')
        refused(run(flownet_args(_lib, enc_dim=100), call()), who, b'unsupported network')
        refused(run(a, call(), ts=None), who, b'null')
        refused(run(a, call(), ts=FAKE + 4), who, b'16-byte aligned')
        refused(run(a, call(), nbytes=2 * saved - 4), who, b'tsaved holds', str(2 * saved).encode())
        b = flownet_args(_lib)
        b.saved = None
        refused(run(b, call()), who, b'null saved')
        c = call()
        c.n = 0
        refused(run(a, c), who, b'0 points')
        c.n = (1 << 22) + 1
        refused(run(a, c), who, b'4194305 points')
    refused(fwd(a, call(), jac=None), b'flownet_jacobian_forward', b'null jac')
    refused(fwd(a, call(), jac=FAKE + 2), b'flownet_jacobian_forward', b'aligned')
    refused(bwd(a, call(), djac=None), b'flownet_jacobian_backward', b'null djac')
    refused(bwd(a, call(), ws=None), b'flownet_jacobian_backward', b'jac_workspace')
    refused(bwd(a, call(), ws=FAKE + 8), b'flownet_jacobian_backward', b'16-byte aligned')
    refused(bwd(a, call(), wsbytes=need - 4), b'flownet_jacobian_backward', b'jac_workspace holds', str(need).encode())
    # what the plain calls refuse still comes before any launch, under their names
    b = flownet_args(_lib)
    b.w[1] = None
    refused(fwd(b, call()), b'flownet_jacobian_forward', b'null weight')
    refused(bwd(b, call()), b'flownet_backward_points', b'null weight')
    b = flownet_args(_lib)
    b.saved_bytes = 16
    refused(fwd(b, call()), b'flownet_forward', b'saved holds 16 bytes')
    b = flownet_args(_lib)
    b.gw[2] = None
    refused(bwd(b, call()), b'flownet_backward_points', b'null gradient pointer')
    p = flownet_args(_lib, enc_dim=515)
    p.progressive, p.k_active, p.mask = 1, 515, FAKE
    p.workspace = None
    refused(fwd(p, call()), b'flownet_jacobian_forward', b'workspace')


# ---- 5. the trainer and the command lines ----
def _trainer(argv, net='RBF', **kw):
    from sin_inn_amd import flowtrainer
    return flowtrainer.FlowTrainer(G.trainer_args(net=net, argv=argv, **kw))


def _stub_step(model, calls):
    """training_step on the host with the network's grid call and the losses stubbed; flow_at records and answers from the composed form"""
    from sin_inn_amd import flownet
    zero = torch.zeros((), requires_grad=True)

    def forward(frame, times, scale):
        calls.append(('flow_fields', {}))
        flows = torch.zeros(times.numel(), 4, *frame.shape[-2:])
        return flows[:, :2], flows[:, 2:]

    def flow_at(net, poses, scale=1.0, **kw):
        calls.append(('flow_at', dict(kw, n=poses.shape[0])))
        return flownet.flow_jacobian_composed(net, poses, scale, kw['jacobian'], planar=kw['planar'])

    model.forward = forward
    model.losses = lambda f1, f2, a, b: (zero, zero, zero, zero, (None, None, None, None))
    logged = {}
    model.log = lambda name, value, **kw: logged.__setitem__(name, value)
    model._scale = lambda scale, frame: 8.0
    real = flownet.flow_at
    flownet.flow_at = flow_at
    try:
        batch = G.trainer_batch()
        return model.training_step([batch[0], batch[1], batch[2], batch[3]], 0), logged
    finally:
        flownet.flow_at = real


def test_the_step_without_the_switches_is_the_step_it_was_and_with_them_one_extra_call():
    for argv in ([], ['--loss-smooth-at', '0', '--smooth-points', '64'], ['--smooth-points', '64']):
        model = _trainer(argv)
        assert model.smooth_at_weight == 0 and not hasattr(model, 'loss_smooth_at') and not hasattr(model, 'smooth_points')
        calls = []
        _, logged = _stub_step(model, calls)
        assert calls == [('flow_fields', {})] and 'train/smooth_at' not in logged
    for net in ('RBF', 'PRBF'):
        model = _trainer(['--loss-smooth-at', '0.5', '--smooth-points', '64'], net=net)
        assert model.loss_smooth_at == 0.5 and model.smooth_points == 64
        calls = []
        loss, logged = _stub_step(model, calls)
        assert calls == [('flow_at', dict(planar=True, jacobian='yx', n=64)), ('flow_fields', {})]
        pair, py, px, poses = model.smooth_sample
        assert int(pair.min()) >= 0 and int(pair.max()) <= 2 and float(py.max()) <= 23 and float(px.max()) <= 39 and float(py.min()) >= 0
        assert torch.equal(poses[:, 1], 2 * py / 23 - 1) and torch.equal(poses[:, 2], 2 * px / 39 - 1)
        assert torch.equal(poses[:, 0], G.trainer_batch()[2].to(F32)[pair])
        assert float(logged['train/smooth_at'].detach()) > 0 and torch.equal(loss.detach(), logged['train/smooth_at'].detach())
        loss.backward()
        lin = (model.net.model if hasattr(model.net, 'mask') else model.net).linears()
        assert all(l.weight.grad is not None and bool((l.weight.grad != 0).any()) for l in lin)     # the derivative trains every layer
        # fused = False: the composed form, no flow_at
        model.fused = False
        calls = []
        _stub_step(model, calls)
        assert calls == [('flow_fields', {})]
    # its own generator: one seed, one sequence, and the between draw does not move
    a, b = (_trainer(['--loss-smooth-at', '1', '--smooth-points', '32']) for _ in range(2))
    times = G.trainer_batch()[2]
    first, again = a.smooth_points_table(times, 3, 24, 40), b.smooth_points_table(times, 3, 24, 40)
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    assert not torch.equal(a.smooth_points_table(times, 3, 24, 40)[1], first[1])
    with_between = _trainer(['--loss-smooth-at', '1', '--smooth-points', '32', '--loss-between', '1', '--between-points', '16'], between_dt=2 / 3)
    alone = _trainer(['--loss-between', '1', '--between-points', '16'], between_dt=2 / 3)
    with_between.smooth_points_table(times, 3, 24, 40)
    assert all(torch.equal(x, y) for x, y in zip(with_between.between_points_table(times, 3, 24, 40)[:3], alone.between_points_table(times, 3, 24, 40)[:3]))


def test_the_smoothness_term_is_zero_slope_free_and_edge_aware():
    """a network whose last layer is zero has a zero Jacobian: the term is W * 2 * 0.5 * 2 * mean(w) * 1e-3, below W * 2e-3, and a
    flat guide image gives exactly W * 2e-3 (every edge weight is exp(0))"""
    model = _trainer(['--loss-smooth-at', '0.5', '--smooth-points', '64'])
    with torch.no_grad():
        model.net.linears()[3].weight.zero_()
    model.fused = False
    batch = G.trainer_batch()
    got = model.smooth_at_loss(batch[0], batch[1], batch[2], 8.0)
    assert 0 < float(got.detach()) <= 0.5 * 2e-3 * (1 + 1e-6)
    flat = torch.full_like(batch[0], 0.25)
    got = model.smooth_at_loss(flat, flat, batch[2], 8.0)
    assert abs(float(got.detach()) - 0.5 * 2e-3) < 1e-9


def test_command_lines(capsys):
    m = G.flow_main()
    base = ['train', '--synthetic', '4', '24', '40']
    args = m.get_args(base + ['--loss-smooth-at', '0.1', '--smooth-points', '512', '--net', 'PRBF'])
    assert args.loss_smooth_at == 0.1 and args.smooth_points == 512
    plain = m.get_args(base)
    assert not hasattr(plain, 'loss_smooth_at') and not hasattr(plain, 'smooth_points')         # present only when given
    for net in ('RFF', 'PRBFG', 'PE'):
        with pytest.raises(SystemExit):
            m.get_args(base + ['--loss-smooth-at', '0.1', '--net', net])
        assert f'--net {net}' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        m.get_args(base + ['--loss-smooth-at', '0.1', '--net', 'PRBF', '--spatially-adaptive'])
    assert 'per-point' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        m.get_args(base + ['--loss-smooth-at', '0.1', '--smooth-points', '0'])
    with pytest.raises(ValueError, match='second derivative'):
        _trainer([], net='RFF', loss_smooth_at=1.0)
    import importlib.util
    spec = importlib.util.spec_from_file_location('flow_interp_smooth', os.path.join(G.ROOT, 'video-interpolation', 'interpolate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ibase = ['--synthetic', '4', '24', '40', '--name', 'x', '--net', 'RBF', '--fit-epochs', '1']
    _, args = mod.trainer_args(mod.get_args(ibase + ['--loss-smooth-at', '0.2', '--smooth-points', '128']))
    assert args.loss_smooth_at == 0.2 and args.smooth_points == 128
    _, args = mod.trainer_args(mod.get_args(ibase))
    assert not hasattr(args, 'loss_smooth_at') and not hasattr(args, 'smooth_points')
