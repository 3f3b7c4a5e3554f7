"""GPU: the flow trainer -- the three operators of csrc/flowtrain.hip against float64 / the reference's images, one training step
of FlowTrainer against the float64 evaluation of the same step, and the command line end to end in child processes.

Method (that of tests/test_gpu_flownet.py): the reference of a number is its float64 evaluation on the same inputs, the unit of
error the deviation of the same expression evaluated by torch in fp32 from float64, measured in the test; the code under test is
allowed MULT = 4 units.  Images are compared under the fixture condition of tests/flowtrainer_refs.py (at most 1 value in 10^4
differs, by one level).  Thresholds (occlusion masks, splat != 0) are compared first, on their own; the losses are then evaluated on
the masks the kernels produced, as gradients are with forced gates.
"""
import argparse
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowtrainer_refs as R  # noqa: E402
from sin_inn_amd import flowdata, flowtrainer  # noqa: E402

F64 = torch.float64
MULT = 4.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


# ---- sininn_flow_epe ----

@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 13, 37), (3, 40, 257)])
def test_flow_epe_against_float64(dev, shape):
    """(3, 40, 257): 121 blocks -- more than the finish wave has lanes -- and a ragged last one"""
    from sin_inn_amd import _lib
    n, h, w = shape
    g = torch.Generator().manual_seed(3)
    flows = (torch.randn(n, 4, h, w, generator=g) * 3).to(dev)
    gt = (torch.randn(n, 2, h, w, generator=g) * 3).to(dev)
    blocks = _lib.lib().sininn_flow_epe_partials(n, h, w)
    assert blocks == -(-n * h * w // 256)
    for name, view in (('contiguous', flows[:, :2].contiguous()), ('channels 0..1', flows[:, :2]), ('channels 2..3', flows[:, 2:])):
        ref64 = R.epe_ref(view.to(F64), gt.to(F64))
        ref32 = R.epe_ref(view, gt)
        part = torch.full((blocks,), float('nan'), device=dev, dtype=F64)
        got = flowtrainer.flow_epe(view, gt, part)
        part.fill_(float('nan'))
        again = flowtrainer.flow_epe(view, gt, part)
        assert got.dtype == torch.float32 and got.dim() == 0 and bool(torch.isfinite(got))
        assert torch.equal(got, again), 'two calls differ'
        unit = abs(float(ref32.to(F64) - ref64)) / abs(float(ref64))
        err = abs(float(got.to(F64) - ref64)) / abs(float(ref64))
        print(f'epe {shape} {name}: err {err:.3g}  fp32-torch unit {unit:.3g}  budget {MULT * unit:.3g}')
        assert err <= MULT * unit, (shape, name, err, unit)


def test_flow_epe_refuses_bad_sizes(dev):
    from sin_inn_amd import _lib
    from sin_inn_amd.ops import _stream, ptr
    import ctypes as C
    lib = _lib.lib()
    flow, gt, out = torch.zeros(2, 2, 4, 4, device=dev), torch.zeros(2, 2, 4, 4, device=dev), torch.zeros(1, device=dev)
    part = torch.zeros(1, device=dev, dtype=F64)
    p = C.c_void_p(part.data_ptr())
    assert lib.sininn_flow_epe(ptr(flow), 32, ptr(gt), 2, 4, 4, p, 1, ptr(out), _stream()) == 0
    assert lib.sininn_flow_epe(ptr(flow), 31, ptr(gt), 2, 4, 4, p, 1, ptr(out), _stream()) != 0       # stride below two planes
    assert lib.sininn_flow_epe(ptr(flow), 32, ptr(gt), 2, 4, 4, p, 0, ptr(out), _stream()) != 0       # partial buffer too small
    assert lib.sininn_flow_epe(ptr(flow), 32, ptr(gt), 0, 4, 4, p, 1, ptr(out), _stream()) != 0
    assert lib.sininn_flow_epe_partials(0, 4, 4) == 0
    assert lib.sininn_splat_mask(ptr(gt), 2, ptr(gt), 2, 3, 4, 4, ptr(gt), _stream()) != 0            # 2 mask channels
    assert lib.sininn_splat_mask(ptr(gt), 1, ptr(gt), 2, 2, 4, 4, ptr(gt), _stream()) != 0            # 2 splat channels
    assert lib.sininn_flow2img_workspace_floats(1, 0, 4) == 0
    with pytest.raises(NotImplementedError):
        flowtrainer.flow_epe(flow.cpu(), gt.cpu())


# ---- sininn_splat_mask ----

@pytest.mark.parametrize('cm', [1, 3])
def test_splat_mask_bitwise(dev, cm):
    g = torch.Generator().manual_seed(4)
    splat = torch.randn(2, 3, 13, 37, generator=g)
    splat[torch.rand(2, 3, 13, 37, generator=g) < 0.2] = 0.0
    splat[0, 1, 2, 3], splat[1, 2, 12, 36], splat[1, 0, 0, 0] = -0.0, -0.0, 0.0
    mask = (torch.rand(2, cm, 13, 37, generator=g) > 0.3).float() * (1 + torch.rand(2, cm, 13, 37, generator=g))
    splat, mask = splat.to(dev), mask.to(dev)
    got = flowtrainer.splat_mask(mask, splat)
    want = R.splat_mask_ref(mask, splat)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert float(got[0, 1, 2, 3]) == 0.0 and float(got[1, 2, 12, 36]) == 0.0
    assert torch.equal(flowtrainer.splat_mask(mask.bool(), splat), R.splat_mask_ref(mask.bool().float(), splat))


# ---- sininn_flow2img ----

@pytest.mark.parametrize('case', R.F2I_CASES)
def test_flow2img_against_the_reference_images(dev, case):
    fx = R.fixture()
    flow = torch.from_numpy(fx[f'f2i_{case}_flow']).to(dev)
    got = flowtrainer.flow2img(flow, float(fx[f'f2i_{case}_clip']))
    assert got.dtype == torch.uint8 and got.is_cuda
    R.assert_image_close(got.cpu(), fx[f'f2i_{case}_img'], case)


def test_flow2img_batch_is_per_frame(dev):
    """three frames with maxima 3, 30 (clipped to 10) and 0.5: a maximum shared across the batch would change two of them; the
    wide frame (3 x 1100 pixels) spans more than one block of the maximum pass"""
    g = torch.Generator().manual_seed(6)
    frames = torch.randn(3, 2, 3, 1100, generator=g) * torch.tensor([1.0, 10.0, 0.15]).view(3, 1, 1, 1)
    frames[1, 0, 2, 1099] = 30.0
    frames = frames.to(dev)
    batch = flowtrainer.flow2img(frames)
    assert tuple(batch.shape) == (3, 3, 3, 1100)
    for i in range(3):
        single = flowtrainer.flow2img(frames[i])
        assert torch.equal(batch[i], single), i
        R.assert_image_close(single.cpu(), R.flow2img_ref(frames[i].cpu()), f'frame {i} against the restatement')
    assert not torch.equal(batch[0], batch[2])


# ---- FlowTrainer.training_step ----

def _args(net, occl='wang', **kw):
    d = dict(lr=1e-4, loss_l1=1, loss_census=0.1, loss_ssim=0.05, census_width=3, loss_smooth1=0.1, edge_constant=150, edge_func='gauss',
             occl=occl, occl_thresh=0.7, net=net)
    d.update(kw)
    return argparse.Namespace(**d)


def _net(name, dev):
    from sin_inn_amd import flownet, progressive
    torch.manual_seed(0)
    nets = {**flownet.model_dict, **flownet.progressive_model_dict}
    net = nets[name](flownet.ModelParams())
    if net.is_progressive:
        net = progressive.LinearControllerEarly(net, 1000, epsilon=1e-3)
    return net.to(dev)


CLIP_SEED = 0


@pytest.fixture(scope='module')
def batch(dev):
    clip = flowdata.SyntheticClip(3, 24, 40, seed=CLIP_SEED)
    return [clip.video[0:2].to(dev), clip.video[1:3].to(dev), clip.T[0:2].to(dev), torch.tensor([clip.flow_scale] * 2, dtype=F64).to(dev),
            clip.flow[0:2].to(dev)]


@pytest.mark.parametrize('name', ['RBF', 'PRBF'])
def test_training_step_against_float64(dev, batch, name):
    args = _args(_net(name, dev))
    model = flowtrainer.FlowTrainer(args).to(dev)
    opt = model.attach_optimizer()
    frame1, frame2, times, scale, gt = batch
    with torch.no_grad():                                    # the flows and masks of this step (the controller moves its mask after it)
        flow12, flow21 = (f.contiguous() for f in model(frame1, times, scale))
        *_, (kmask1, kmask2, _, _) = model.losses(frame1, frame2, flow12, flow21)
    opt.zero_grad()
    loss = model.training_step(batch, 0)
    logged = {k: v.detach().to(F64).cpu() for k, v in model._logged.items()}
    assert set(logged) == {'train/EPE', 'train/loss', 'train/loss_epoch', 'train/l1', 'train/census', 'train/ssim', 'train/smooth'}
    assert float(logged['train/loss']) == float(loss)

    cpu = [t.detach().cpu() for t in (frame1, frame2, flow12, flow21)]
    m64 = R.step_masks_ref(*[t.to(F64) for t in cpu], args.occl, args.occl_thresh)[:2]
    m32 = R.step_masks_ref(*cpu, args.occl, args.occl_thresh)[:2]
    for i, (a, b, k) in enumerate(zip(m64, m32, (kmask1, kmask2))):
        oracle_diff = float((a.to(torch.float32) != b).float().mean())
        kernel_diff = float((a.to(torch.float32) != k.cpu()).float().mean())
        print(f'{name} mask{i + 1}: fp32 oracle differs from float64 on {oracle_diff:.3%} of pixels, the kernels on {kernel_diff:.3%}; '
              f'open {float(a.mean()):.3f}')
        assert oracle_diff == 0.0, 'CLIP_SEED: the oracle itself sits on a threshold'
        assert kernel_diff <= 0.005
    kmasks = (kmask1.cpu(), kmask2.cpu())
    ref64, _ = R.step_losses_ref(*[t.to(F64) for t in cpu], args, masks=kmasks)
    ref32, _ = R.step_losses_ref(*cpu, args, masks=kmasks)
    ref64['EPE'], ref32['EPE'] = R.epe_ref(cpu[2].to(F64), gt.cpu().to(F64)), R.epe_ref(cpu[2], gt.cpu())
    failures = []
    for term in ('loss', 'l1', 'census', 'ssim', 'smooth', 'EPE'):
        want = float(ref64[term])
        unit = abs(float(ref32[term].to(F64)) - want) / abs(want)
        err = abs(float(logged[f'train/{term}']) - want) / abs(want)
        print(f'{name} {term}: value {want:.6g}  err {err:.3g}  fp32-torch unit {unit:.3g}  budget {MULT * unit:.3g}')
        if not err <= MULT * unit:
            failures.append((term, err, MULT * unit))
    assert not failures, failures

    loss.backward()
    params = list(model.net.parameters())
    assert len(params) == 8
    for p in params:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    before = [p.detach().clone() for p in params]
    opt.step()
    for p, b in zip(params, before):
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), b)


@pytest.mark.parametrize('occl', [None, 'brox'])
def test_training_step_other_occlusions(dev, batch, occl):
    model = flowtrainer.FlowTrainer(_args(_net('RBF', dev), occl=occl, loss_ssim=0)).to(dev)
    model.attach_optimizer().zero_grad()
    loss = model.training_step(batch[:4], 0)                 # no ground truth: four entries
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    assert 'train/EPE' not in model._logged and 'train/ssim' not in model._logged
    loss.backward()
    fused = float(loss)
    model.fused = False                                      # the torch expressions of the operators: the same step
    assert abs(float(model.training_step(batch[:4], 0)) - fused) <= 1e-5 * fused


# ---- the command line, in child processes ----

def _run(cwd, *argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'video-interpolation', 'main.py'), *argv], cwd=cwd, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, argv
    return r.stdout


def test_command_line_end_to_end(dev, tmp_path):
    from PIL import Image
    cwd = str(tmp_path)
    common = ['--synthetic', '4', '24', '40', '--net', 'PRBF', '--batch', '2', '--wandb', 'x', '--name', 't']
    _run(cwd, 'train', *common, '--epochs', '6', '--val-iter', '3')
    log = os.path.join(cwd, 'x_synthetic_t.jsonl')
    records = [json.loads(line) for line in open(log)]
    epochs = [r for r in records if 'train/loss_epoch' in r and 'wall_s' not in r and 'test/EPE' not in r]
    assert [r['step'] for r in epochs] == [2, 4, 6, 8, 10, 12]
    print('epoch losses', [r['train/loss_epoch'] for r in epochs])
    assert epochs[5]['train/loss_epoch'] < epochs[0]['train/loss_epoch']
    assert len([r for r in records if 'wall_s' in r and 'val/EPE' in r]) == 2
    ckpts = sorted(os.listdir(os.path.join(cwd, 'checkpoints', 'synthetic', 't')))
    assert ckpts == [f'epoch={e}.ckpt' for e in range(6)]
    ck = torch.load(os.path.join(cwd, 'checkpoints', 'synthetic', 't', 'epoch=5.ckpt'), map_location='cpu')
    assert 'net.mask_stashed' in ck['state_dict'] and all(k.startswith('net.') for k in ck['state_dict'])
    assert float(ck['state_dict']['net.mask_stashed'][0]) == 78.0            # 12 steps, one block of 6 per step after the first
    assert ck['optimizer_states'][0]['flat'][0]['step'] == 12 and ck['global_step'] == 12

    out = _run(cwd, 'test', *common)
    gifs = [f for f in os.listdir(os.path.join(cwd, 'results')) if f.startswith('flow_synthetic_t_epe_')]
    assert len(gifs) == 1 and os.path.isfile(os.path.join(cwd, 'results', 'occl_synthetic_t.gif'))
    with Image.open(os.path.join(cwd, 'results', gifs[0])) as im:
        assert im.n_frames == 3 and im.size == (40, 24)
    tests = [json.loads(line) for line in open(log)]
    tests = [r['test/EPE'] for r in tests if 'test/EPE' in r]
    assert len(tests) == 2                                                   # after training, and from `test`
    assert gifs[0] == f'flow_synthetic_t_epe_{tests[-1]:.3f}.gif' and f'test/EPE {tests[-1]:.6f}' in out

    out = _run(cwd, 'train', *common, '--epochs', '8')                       # resumes from epoch=5.ckpt at epoch 6
    assert 'resumed: iteration 12, controller cur_block 78 / 515' in out
    records = [json.loads(line) for line in open(log)]
    assert [r['step'] for r in records if 'train/loss_epoch' in r and 'wall_s' not in r and r['step'] > 12] == [14, 16]
    assert sorted(os.listdir(os.path.join(cwd, 'checkpoints', 'synthetic', 't')))[-2:] == ['epoch=6.ckpt', 'epoch=7.ckpt']

    _run(cwd, 'sintel', *common)
    outdir = os.path.join(cwd, 'sintel_submission', 'final', 'synthetic')
    assert sorted(os.listdir(outdir)) == ['frame_0001.flo', 'frame_0002.flo', 'frame_0003.flo']
    import importlib.util
    spec = importlib.util.spec_from_file_location('flow_main', os.path.join(ROOT, 'video-interpolation', 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    args = m.get_args(['sintel', *common])
    args.net = m.build_net(args)
    model = flowtrainer.FlowTrainer.load_from_checkpoint(os.path.join(cwd, 'checkpoints', 'synthetic', 't', 'epoch=7.ckpt'), args=args).to(dev)
    clip = flowdata.SyntheticClip(4, 24, 40)
    with torch.no_grad():
        for i in range(3):
            f1, _, t, s = clip[i][:4]
            flow, _ = model(f1.to(dev)[None], t.to(dev)[None], s)
            back = flowdata.readFlow(os.path.join(outdir, f'frame_{i + 1:04d}.flo'))
            assert torch.equal(torch.from_numpy(back), flow[0].permute(1, 2, 0).cpu()), i
