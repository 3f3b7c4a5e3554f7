"""CPU: the host side of the flow trainer -- the flow2img restatement against the reference's own images, .flo IO against the
reference's bytes, the Images / SyntheticClip data sets, the command line's defaults and refusals, and the trainer stand-in's
automatic-optimisation path.  Fixtures: tests/golden/golden_flowtrainer.npz (tests/golden/make_golden_flowtrainer.py).
"""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowtrainer_refs as R  # noqa: E402
from sin_inn_amd import flowdata, flowtrainer  # noqa: E402
from sin_inn_amd.lightning import LightningDataModule, LightningModule, Trainer  # noqa: E402


def flow_main():
    spec = importlib.util.spec_from_file_location('flow_main', os.path.join(ROOT, 'video-interpolation', 'main.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('case', R.F2I_CASES)
def test_flow2img_restatement_reproduces_the_reference(case):
    """at most 1 value in 10^4 differs from the reference's image, by one level (measured here: none differs in any case)"""
    fx = R.fixture()
    got = R.flow2img_ref(torch.from_numpy(fx[f'f2i_{case}_flow']), float(fx[f'f2i_{case}_clip']))
    R.assert_image_close(got, fx[f'f2i_{case}_img'], case)
    if case == 'zero':
        assert int(got.max()) == 0


def test_color_wheel_is_the_restated_one():
    wheel = flowtrainer.make_color_wheel()
    assert wheel.shape == (55, 3) and wheel.dtype == np.float64
    assert np.array_equal(wheel, R.color_wheel_ref().numpy())


def test_flo_round_trip_against_the_reference_bytes(tmp_path):
    fx = R.fixture()
    fn = str(tmp_path / 'field.flo')
    flowdata.writeFlow(fn, fx['flo_field'])
    assert open(fn, 'rb').read() == fx['flo_bytes'].tobytes()
    back = flowdata.readFlow(fn)
    assert back.dtype == np.float32 and np.array_equal(back, fx['flo_read'])
    flowdata.writeFlow(fn, fx['flo_field'][:, :, 0], fx['flo_field'][:, :, 1])
    assert open(fn, 'rb').read() == fx['flo_bytes'].tobytes()
    bad = bytearray(fx['flo_bytes'].tobytes())
    bad[0] ^= 0xff
    open(fn, 'wb').write(bytes(bad))
    assert flowdata.readFlow(fn) is None


def _write_scene(root, with_flow, h=40, w=64, frames=6):
    from PIL import Image
    scene = root / 'final' / 'scene_1'
    scene.mkdir(parents=True)
    g = torch.Generator().manual_seed(5)
    for i in range(frames):
        Image.fromarray((torch.rand(h, w, 3, generator=g) * 255).to(torch.uint8).numpy()).save(scene / f'frame_{i + 1:04d}.png')
    flows = []
    if with_flow:
        fdir = root / 'flow' / 'scene_1'
        fdir.mkdir(parents=True)
        for i in range(frames - 1):
            flows.append((torch.randn(h, w, 2, generator=g) * 2).numpy())
            flowdata.writeFlow(str(fdir / f'frame_{i + 1:04d}.flo'), flows[-1])
    return str(scene), flows


def test_images_with_ground_truth(tmp_path):
    scene, flows = _write_scene(tmp_path, True)
    ds = flowdata.Images(scene, size=20)
    assert len(ds) == 5 and ds.gt_available
    assert tuple(ds.video.shape) == (6, 3, 20, 32) and tuple(ds.flow.shape) == (5, 2, 20, 32)
    assert ds.flow_scale == 32 / 5
    assert torch.equal(ds.T, torch.linspace(-1, 1, 6))
    for i in range(5):
        item = ds[i]
        assert len(item) == 5
        assert torch.equal(item[0], ds.video[i]) and torch.equal(item[1], ds.video[i + 1])
        assert float(item[2]) == float(ds.T[i]) and item[3] == ds.flow_scale and torch.equal(item[4], ds.flow[i])
    assert float(ds.video.min()) >= 0 and float(ds.video.max()) <= 1
    # ground truth: resized like the frames, then multiplied by size / h (here 1 / 2) so that it stays in pixels
    want = torch.stack([flowdata.resize_shorter_side(torch.tensor(f).permute(2, 0, 1), 20) for f in flows]) * (20 / 40)
    assert torch.equal(ds.flow, want)
    full = flowdata.Images(scene, size=40)                      # size == h: nothing is resampled, the scale is 1
    assert torch.equal(full.flow, torch.stack([torch.tensor(f).permute(2, 0, 1) for f in flows]))
    assert full.flow_scale == 64 / 5


def test_images_without_ground_truth(tmp_path):
    scene, _ = _write_scene(tmp_path, False)
    ds = flowdata.Images(scene, size=20)
    assert len(ds) == 5 and not ds.gt_available
    assert all(len(ds[i]) == 4 for i in range(5))


def _warp_back(img, flow):
    """img sampled at x + flow(x), bilinear"""
    n, c, h, w = img.shape
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    gx = (xx[None] + flow[:, 0]) / (w - 1) * 2 - 1
    gy = (yy[None] + flow[:, 1]) / (h - 1) * 2 - 1
    return torch.nn.functional.grid_sample(img, torch.stack((gx, gy), -1), mode='bilinear', padding_mode='border', align_corners=True)


def test_synthetic_clip_ground_truth_is_a_flow_of_the_clip():
    """frame i + 1 sampled at x + flow_i(x) is frame i, 4 pixels inside the border.  The bound is what the same check gives for
    tools/fit_flow.make_pair at the same size (24 x 40, seed 1): 0.0158 there (bilinear sampling of the texture, and make_pair's
    flow is the displacement at the target, not the source); the clip measures 0.0048."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fit_flow
    h, w = 24, 40
    f1, f2, flow = fit_flow.make_pair(h, w, 1, 'cpu')
    bound = float((_warp_back(f2, flow) - f1).abs()[:, :, 4:-4, 4:-4].max())
    clip = flowdata.SyntheticClip(4, h, w, seed=1)
    assert len(clip) == 3 and len(clip[0]) == 5 and clip.gt_available and clip.flow_scale == w / 5
    assert torch.equal(clip.T, torch.linspace(-1, 1, 4))
    assert clip.video.dtype == torch.float32 and tuple(clip.video.shape) == (4, 3, h, w) and tuple(clip.flow.shape) == (3, 2, h, w)
    worst = max(float((_warp_back(clip.video[i + 1:i + 2], clip.flow[i:i + 1]) - clip.video[i:i + 1]).abs()[:, :, 4:-4, 4:-4].max())
                for i in range(3))
    print(f'make_pair {bound:.4g}  clip {worst:.4g}')
    assert 0.01 < bound < 0.02 and worst <= bound
    assert float(clip.flow.abs().max()) > 0.3                                  # the clip moves
    pair = flowdata.SyntheticClip(2, h, w, seed=1)                             # two frames: make_pair's pair
    assert float((pair.video[0:1] - f1).abs().max()) < 1e-5 and float((pair.video[1:2] - f2).abs().max()) < 1e-5


REFERENCE_DEFAULTS = dict(ngpus=1, input_video='../datasets/sintel/training/final/alley_1', name='temp', end=None, step=None, size=436,
                          batch=1, test_size=436, test_batch=1, net='RBF', spatially_adaptive=False, epochs=1000, val_iter=None, lr=1e-4,
                          loss_l1=1, loss_census=0.1, loss_ssim=0, census_width=3, loss_smooth1=0.1, edge_constant=150, edge_func='gauss',
                          occl='wang', occl_thresh=0.7, wandb=None, log_gt=False)


def test_cli_defaults_are_the_references():
    """video-interpolation/main.py:17-49 of the reference, option by option"""
    m = flow_main()
    for op in ('train', 'test', 'summarize', 'sintel'):
        args = vars(m.get_args([op]))
        assert args.pop('operation') == op
        assert args.pop('synthetic') is None
        assert args == REFERENCE_DEFAULTS
    args = m.get_args(['train', '--synthetic', '4', '24', '40', '--net', 'PRBF', '--wandb', 'anything', '--occl', 'None'])
    assert args.synthetic == [4, 24, 40] and args.wandb == 'anything' and args.occl is None


@pytest.mark.parametrize('argv, needle', [(['train', '--spatially-adaptive'], 'out of scope'), (['train', '--net', 'siren'], 'out of scope'),
                                          (['train', '--net', 'MPFF'], 'out of scope'), (['train', '--net', 'nonsense'], 'unknown network')])
def test_cli_refuses_what_the_port_does_not_have(argv, needle, capsys):
    m = flow_main()
    with pytest.raises(SystemExit) as e:
        m.get_args(argv)
    assert e.value.code == 2
    assert needle in capsys.readouterr().err


class _Counting(torch.optim.SGD):
    def __init__(self, params):
        super().__init__(params, lr=0.1)
        self.calls = []

    def zero_grad(self, set_to_none=False):
        self.calls.append('zero_grad')
        super().zero_grad(set_to_none=set_to_none)

    def step(self, *a, **kw):
        self.calls.append('step')
        return super().step(*a, **kw)


class _Toy(LightningModule):
    def __init__(self, manual):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(3))
        self.automatic_optimization = not manual
        self.backwards = 0
        self.ended = False

    def training_step(self, batch, batch_idx):
        loss = ((self.w * batch[0]).sum() - 1) ** 2
        loss.register_hook(lambda g: setattr(self, 'backwards', self.backwards + 1))
        if not self.automatic_optimization:
            return {'loss': loss.detach()}
        return loss

    def on_train_end(self):
        self.ended = True

    def configure_optimizers(self):
        self.opt = _Counting(self.parameters())
        return self.opt


class _ToyData(LightningDataModule):
    def train_dataloader(self):
        return [(torch.full((3,), float(i + 1)),) for i in range(4)]


def test_trainer_automatic_optimisation_once_per_batch():
    model = _Toy(manual=False)
    before = model.w.detach().clone()
    Trainer(max_epochs=2, accelerator='cpu').fit(model, _ToyData())
    assert model.opt.calls == ['zero_grad', 'step'] * 8                      # 2 epochs x 4 batches, in this order
    assert model.backwards == 8
    assert not torch.equal(model.w.detach(), before) and model.ended


def test_trainer_leaves_a_manual_module_alone():
    model = _Toy(manual=True)
    before = model.w.detach().clone()
    Trainer(max_epochs=2, accelerator='cpu').fit(model, _ToyData())
    assert model.opt.calls == [] and model.backwards == 0
    assert torch.equal(model.w.detach(), before)

    class ManualTensor(_Toy):                                                # opted out, and returns a tensor that requires grad
        def training_step(self, batch, batch_idx):
            loss = ((self.w * batch[0]).sum() - 1) ** 2
            loss.register_hook(lambda g: setattr(self, 'backwards', self.backwards + 1))
            return loss

    model = ManualTensor(manual=True)
    Trainer(max_epochs=1, accelerator='cpu').fit(model, _ToyData())
    assert model.opt.calls == [] and model.backwards == 0


def test_trainer_test_loop_runs_test_step_then_test_epoch_end():
    class T(_Toy):
        def test_step(self, batch, batch_idx):
            assert not torch.is_grad_enabled()
            return float(batch[0][0]) + batch_idx

        def test_epoch_end(self, outputs):
            return outputs

    class D(_ToyData):
        def test_dataloader(self):
            return self.train_dataloader()

    assert Trainer(accelerator='cpu').test(T(manual=False), D()) == [1.0, 3.0, 5.0, 7.0]
    assert LightningDataModule().test_dataloader() is None


def test_resume_restores_the_controller_schedule():
    """on_load_checkpoint: iteration from the global step, cur_block from mask_stashed but never ahead of the schedule"""
    m = flow_main()
    args = m.get_args(['train', '--net', 'PRBF', '--epochs', '6'])
    args.net = m.build_net(args)
    assert args.net.block_iterations == 1                                    # below 112 epochs: one block per step
    for _ in range(12):
        args.net.stash_iteration(torch.tensor(1.0))
    assert args.net.cur_block == 78
    src = flowtrainer.FlowTrainer(args)
    sd = src.state_dict()
    assert float(sd['net.mask_stashed'][0]) == 78.0
    args2 = m.get_args(['train', '--net', 'PRBF', '--epochs', '6'])
    args2.net = m.build_net(args2)
    dst = flowtrainer.FlowTrainer(args2)
    dst.load_state_dict(sd)
    dst.on_load_checkpoint({'global_step': 12})
    assert dst.net.cur_block == 78 and dst.net.next_block == 84 and dst.net.iteration == 12
    assert torch.equal(dst.net.mask, src.net.mask)
    # a long schedule, half way through a ramp that has reached 1: the sum counts the block as open, the schedule does not yet
    args3 = m.get_args(['train', '--net', 'PRBF', '--epochs', '1120'])
    args3.net = m.build_net(args3)
    assert args3.net.block_iterations == 10
    for _ in range(27):
        args3.net.stash_iteration(torch.tensor(1.0))
    assert args3.net.cur_block == 18 and float(args3.net.mask.sum()) == 24.0
    sd = flowtrainer.FlowTrainer(args3).state_dict()
    args4 = m.get_args(['train', '--net', 'PRBF', '--epochs', '1120'])
    args4.net = m.build_net(args4)
    dst = flowtrainer.FlowTrainer(args4)
    dst.load_state_dict(sd)
    dst.on_load_checkpoint({'global_step': 27})
    assert dst.net.cur_block == 18 and dst.net.next_block == 24 and torch.equal(dst.net.mask, args3.net.mask)


def test_latest_checkpoint_breaks_equal_times_by_epoch(tmp_path, monkeypatch):
    """two epochs of a short run can be saved within one tick of the file system's clock; `test`, `sintel` and a resuming `train` must
    then take the later epoch, whatever order glob lists them in.  A later time still wins over a higher epoch"""
    m = flow_main()
    folder = tmp_path / 'checkpoints' / 'scene' / 'run'
    folder.mkdir(parents=True)
    for epoch in (10, 9, 6, 7):
        (folder / f'epoch={epoch}.ckpt').write_bytes(b'')
        os.utime(folder / f'epoch={epoch}.ckpt', (1000, 1000))
    monkeypatch.chdir(tmp_path)
    assert os.path.basename(m._latest_ckpt('scene', 'run')) == 'epoch=10.ckpt'
    os.utime(folder / 'epoch=6.ckpt', (2000, 2000))
    assert os.path.basename(m._latest_ckpt('scene', 'run')) == 'epoch=6.ckpt'
    with pytest.raises(ValueError):
        m._latest_ckpt('scene', 'none')
