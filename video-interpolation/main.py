"""Command line of the flow path, MI355X build: the operations and flags of the reference's video-interpolation/main.py:17-49,
driving `sin_inn_amd.flowtrainer.FlowTrainer`.

    python video-interpolation/main.py train --input-video <sintel scene folder> --batch 3 --epochs 5000
    python video-interpolation/main.py train --synthetic 8 436 1024 --batch 3 --epochs 2
    python video-interpolation/main.py test | summarize | sintel ...

Differences from the reference, all to make the path runnable here:
  * the trainer, checkpoint callback and logger come from `sin_inn_amd.lightning` (pytorch_lightning and wandb are not installed):
    `--wandb NAME` takes any name and writes JSON lines to ./NAME_<scene>_<name>.jsonl, one record per epoch;
  * `--synthetic T H W` trains and tests on `SyntheticClip(T, H, W)`, scene name `synthetic`; no data set is needed;
  * `--layered T H W` does the same on `LayeredClip(T, H, W)`, two moving layers with real occlusion, scene name `layered`;
  * `--holdout S` fits (train) or evaluates (test) on every S-th frame of the clip only (`sin_inn_amd.flowdata.Holdout`); validation
    then logs `val/PSNR` and `val/SSIM` of the synthesized held-out frames in place of `val/EPE`; the attribute exists only when
    the flag is given;
  * `--net` takes the networks that the table of sin_inn_amd/flowcaps.py opens (`cli`); the others exit with a message;
  * `--spatially-adaptive` puts a network with the table's `spatial` under `StashedSpatialController(net, 50, block_iterations)`; with any
    other network it exits with a message.  The reference's own run of this switch fails at the first step (its trainer hands the
    controller a scalar loss) and never calls `update_progress`; here the trainer stashes a per-point loss after every backward pass
    and closes / opens cells every `block_iterations` steps (sin_inn_amd/flowtrainer.py);
  * `--ngpus N` is N devices (cuda:0 .. cuda:N-1, the first is used), as in Lightning, not a device index;
  * a video file as `--input-video` (imageio + RAFT) is refused;
  * LinearControllerEarly(net, epochs) computes `block_iterations = 3 * epochs // (4 * 84)` (PPE: `// 12`), which is 0 below 112 (4) epochs, and the
    reference then divides by it; here such a short run opens one block per step;
  * checkpoints are written every max(epochs // 100, 1) epochs (the reference's `every_n_epochs=0` below 100 epochs writes none)
    whenever `--wandb` is given, `test` and `sintel` load the newest one, and `train` resumes from it;
  * `--loss-between W` (with `--between-taus K`, `--between-back {network,reverse}`) adds the in-between consistency loss of
    sin_inn_amd/flowtrainer.py to the training step; the default 0 leaves the step as it was.  `--between-points N` in
    place of `--between-taus` draws it at N random points a step.
  * `--loss-smooth-at W --smooth-points N` adds the edge-aware smoothness prior on the network's analytic Jacobian at N random points a
    step (`train/smooth_at`); the networks with the table's `jacobian`, without --spatially-adaptive.
"""
import argparse
import importlib.util
import os
import os.path as path
import sys
from glob import glob

ROOT = path.dirname(path.dirname(path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location('flowcaps', path.join(ROOT, 'sin-inn_amd', 'flowcaps.py'))
flowcaps = importlib.util.module_from_spec(_spec)              # by path: the package around it imports torch, parsing does not
_spec.loader.exec_module(flowcaps)
NETWORKS = flowcaps.names(cli=True)                            # the twelve --net opens
OUT_OF_SCOPE_NETWORKS = flowcaps.names(cli=False)              # siren, MPFF
JACOBIAN_NETWORKS = flowcaps.names('jacobian', cli=True)       # the networks with tangent kernels: --loss-smooth-at
SPATIAL_NETWORKS = flowcaps.names('spatial', cli=True)         # the 515-wide progressive networks of NETWORKS: --spatially-adaptive


def get_parser():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('operation', choices=['train', 'test', 'summarize', 'sintel'])
    parser.add_argument('--ngpus', default=1, type=int)
    # Data options
    parser.add_argument('--input-video', default='../datasets/sintel/training/final/alley_1')
    parser.add_argument('--name', default='temp')
    parser.add_argument('--end', type=int)
    parser.add_argument('--step', type=int)
    parser.add_argument('--size', default=436, type=int)
    parser.add_argument('--batch', default=1, type=int)
    parser.add_argument('--test-size', default=436, type=int)
    parser.add_argument('--test-batch', default=1, type=int)
    parser.add_argument('--synthetic', nargs=3, type=int, metavar=('T', 'H', 'W'),
                        help='train / test on a synthetic clip of T frames of H x W instead of --input-video')
    parser.add_argument('--layered', nargs=3, type=int, metavar=('T', 'H', 'W'), default=argparse.SUPPRESS,
                        help='train / test on a LayeredClip of T frames of H x W (two layers, real occlusion) instead of --input-video')
    parser.add_argument('--holdout', type=int, metavar='S', default=argparse.SUPPRESS,
                        help='keep every S-th frame, hold the others out and score their synthesis (val/PSNR, val/SSIM)')
    # Network options
    parser.add_argument('--net', default='RBF')
    parser.add_argument('--spatially-adaptive', action='store_true')
    # Train options
    parser.add_argument('--epochs', default=1000, type=int)
    parser.add_argument('--val-iter', type=int)
    parser.add_argument('--lr', default=1e-4, type=float)
    parser.add_argument('--loss-l1', default=1, type=float)
    parser.add_argument('--loss-census', default=0.1, type=float)
    parser.add_argument('--loss-ssim', default=0, type=float)
    parser.add_argument('--census-width', default=3, type=int)
    parser.add_argument('--loss-smooth1', default=0.1, type=float)
    parser.add_argument('--edge-constant', default=150, type=float)
    parser.add_argument('--edge-func', default='gauss', choices=['exp', 'gauss'])
    parser.add_argument('--occl', default='wang', choices=['brox', 'wang', 'None', None],
                        help="'None' on the command line stands for the reference's None (no occlusion masks)")
    parser.add_argument('--occl-thresh', default=0.7, type=float)
    # like --holdout, the three attributes exist only when their flag is given: the default namespace stays the reference's
    parser.add_argument('--loss-between', default=argparse.SUPPRESS, type=float, metavar='W',
                        help='weight of the photometric consistency loss at random in-between times (default 0: off, the step as it was)')
    parser.add_argument('--between-taus', default=argparse.SUPPRESS, type=int, metavar='K',
                        help='--loss-between: in-between times drawn per step (default 1)')
    parser.add_argument('--between-back', default=argparse.SUPPRESS, choices=['network', 'reverse'],
                        help="--loss-between: the flow toward the previous frame, as interpolate.py's --back (default network)")
    parser.add_argument('--between-points', default=argparse.SUPPRESS, type=int, metavar='N',
                        help='--loss-between: draw the term at N random (pair, tau, y, x) a step instead of whole frames (DESIGN 23)')
    parser.add_argument('--loss-smooth-at', default=argparse.SUPPRESS, type=float, metavar='W',
                        help='weight of the edge-aware smoothness prior on the analytic flow Jacobian at random points (DESIGN 24; default 0: off)')
    parser.add_argument('--smooth-points', default=argparse.SUPPRESS, type=int, metavar='N',
                        help='--loss-smooth-at: random (pair, y, x) a step (default 4096)')
    # Logging options
    parser.add_argument('--wandb', help='any name: selects the JSON-lines FileLogger and checkpointing')
    parser.add_argument('--log-gt', action='store_true')
    return parser


def get_args(argv=None):
    """the parsed arguments; exits (status 2, with the limitation named) on a network or controller this project does not have"""
    parser = get_parser()
    args = parser.parse_args(argv)
    if args.occl == 'None':                                    # argparse cannot produce the reference's `None` choice from a string
        args.occl = None
    if args.synthetic and getattr(args, 'layered', None):
        parser.error('--synthetic and --layered both name the clip: give one of them')
    if getattr(args, 'holdout', 2) < 2:
        parser.error('--holdout S: S >= 2 (every S-th frame is kept)')
    try:
        flowcaps.check_step_options(args)
    except ValueError as e:
        parser.error(str(e))
    if getattr(args, 'loss_smooth_at', 0) != 0:
        if args.net not in JACOBIAN_NETWORKS:
            parser.error(f'--loss-smooth-at with --net {args.net} is out of scope: the flow Jacobian is built for '
                         f'{", ".join(JACOBIAN_NETWORKS)} (sin_inn_amd/flownet.py, flow_at(.., jacobian=))')
        if args.spatially_adaptive:
            parser.error('--loss-smooth-at with --spatially-adaptive is out of scope: the flow Jacobian takes a global mask, no per-point one')
    if args.spatially_adaptive and args.net not in SPATIAL_NETWORKS:
        parser.error(f'--spatially-adaptive with --net {args.net} is out of scope here: the per-point masks of '
                     f'sin_inn_amd.progressive.StashedSpatialController are built for the 515-wide progressive networks '
                     f'({", ".join(SPATIAL_NETWORKS)})')
    if args.net in OUT_OF_SCOPE_NETWORKS:
        parser.error(f'--net {args.net} is out of scope: the fused kernels are built for {", ".join(NETWORKS)} '
                     '(sin_inn_amd/flownet.py)')
    if args.net not in NETWORKS:
        parser.error(f'--net {args.net}: unknown network; choose from {", ".join(NETWORKS)}')
    return args


def build_net(args, res=50):
    """main.py:136-143: the network, and LinearControllerEarly around a progressive one.  `args.net` is the network's name on the
    first call; main() replaces it with the module, as the reference does, and keeps the name in `args.net_name`.
    With --spatially-adaptive: StashedSpatialController(net, res, block_iterations, epsilon=1e-3), built on the device the trainer
    uses (its grid of masks is res^3 x 515 floats, 257 MB at the reference's res = 50; `res` is a keyword for callers and tests, not
    an option).  `block_iterations = max(3 * epochs // (4 * 84), 1)` is the block length LinearControllerEarly gets for the same run,
    so both switches open the spectrum over the same span of steps; the reference passes `args.epochs` here, a block that no run
    finishes, and never advances."""
    from sin_inn_amd import flownet, progressive
    if isinstance(args.net, str):
        args.net_name = args.net
    net = flownet.all_model_dict[args.net_name](flownet.ModelParams())
    if getattr(args, 'spatially_adaptive', False):
        import torch
        if torch.cuda.is_available():
            net = net.to(torch.device('cuda', _devices(args)[0]))
        return progressive.StashedSpatialController(net, res, block_iterations=max(3 * args.epochs // (4 * 84), 1), epsilon=1e-3)
    if net.is_progressive:
        net = progressive.LinearControllerEarly(net, args.epochs, epsilon=1e-3)
        if net.block_iterations == 0:                          # fewer than 112 epochs (PPE: 4): the reference divides by zero here
            net.block_iterations = 1
            net.progress_iterations = (net.encoding_dim - net.block_size) // net.block_size
    return net


def _devices(args):
    return list(range(max(args.ngpus, 1)))


def _latest_ckpt(scene, name):
    """the newest checkpoint of a run (main.py:86-87); raises like the reference if there is none.  Two epochs of a short run can be
    saved within one tick of the file system's clock: equal times are decided by the epoch in the name, not by the order of glob"""
    def age(ckpt):
        epoch = path.basename(ckpt)[len('epoch='):-len('.ckpt')]
        return path.getmtime(ckpt), int(epoch) if path.basename(ckpt).startswith('epoch=') and epoch.isdigit() else -1
    return max(glob(path.join('checkpoints', scene, name, '*.ckpt')), key=age)


def train_model(args):
    """main.py:52-80"""
    import torch
    from sin_inn_amd.flowdata import get_video
    from sin_inn_amd.flowtrainer import FlowTrainer, flow2img, save_gif
    from sin_inn_amd.lightning import FileLogger, ModelCheckpoint, Trainer
    video, scene = get_video(args.input_video, args)
    dataset = video.testset
    if not args.val_iter:
        args.val_iter = args.epochs + 1
    if getattr(args, 'loss_between', 0) != 0:
        args.between_dt = 2 / (len(dataset.T) - 1)             # the clip being fitted: under --holdout the kept frames

    logger, latest_ckpt, clbks = None, None, []
    if args.wandb:
        logger = FileLogger(project=args.wandb, name=f'{scene}_{args.name}')
        logger.log_hyperparams(argparse.Namespace(**{k: v for k, v in vars(args).items() if k != 'net'}))
        ckpt_dir = path.join('checkpoints', scene, args.name)
        clbks = [ModelCheckpoint(period=max(args.epochs // 100, 1), dirpath=ckpt_dir)]
        latest_ckpt = max(glob(path.join(ckpt_dir, '*.ckpt')), default=None, key=path.getmtime)
    if args.log_gt:                                            # the reference uploads two videos; here they are GIFs
        os.makedirs('results', exist_ok=True)
        save_gif(f'results/source_{scene}_{args.name}.gif', (dataset.video * 255).type(torch.uint8).permute(0, 2, 3, 1).numpy())
        if dataset.gt_available:
            save_gif(f'results/gt_flow_{scene}_{args.name}.gif', flow2img(dataset.flow.cuda()).permute(0, 2, 3, 1).cpu().numpy())

    model = FlowTrainer(args, test_tag=f'{scene}_{args.name}')
    steps_per_epoch = max(len(video.train_dataloader()), 1)
    trainer = Trainer(gpus=_devices(args), logger=logger, max_epochs=args.epochs, callbacks=clbks,
                      resume_from_checkpoint=latest_ckpt, check_val_every_n_epoch=args.val_iter,
                      log_every_n_steps=steps_per_epoch)
    if latest_ckpt:
        print(f'resuming from {latest_ckpt}')
    trainer.fit(model, video)
    if model.completed_training:
        trainer.test(model, video)


def test_model(args):
    """main.py:83-93"""
    from sin_inn_amd.flowdata import get_video
    from sin_inn_amd.flowtrainer import FlowTrainer
    from sin_inn_amd.lightning import FileLogger, Trainer
    video, scene = get_video(args.input_video, args)
    unique_name = f'{scene}_{args.name}'
    latest_ckpt = _latest_ckpt(scene, args.name)
    model = FlowTrainer.load_from_checkpoint(latest_ckpt, args=args, test_tag=unique_name)
    logger = FileLogger(project=args.wandb, name=unique_name) if args.wandb else None
    trainer = Trainer(gpus=_devices(args), logger=logger)
    trainer.test(model, video)
    flow_files = [path.join('results', f) for f in os.listdir('results') if f.startswith(f'flow_{unique_name}_epe')]
    return flow_files, len(video.testset)


def summarize_model(args):
    """main.py:96-106: the frame-weighted mean EPE over every scene beside --input-video"""
    root = path.dirname(args.input_video)
    epe_accum, frame_accum = 0, 0
    for scene in sorted(os.listdir(root)):
        args.input_video = path.join(root, scene)
        args.net = build_net(args)
        files, num_frames = test_model(args)
        assert len(files) == 1
        epe = float(path.splitext(files[0])[0].split('_')[-1])
        epe_accum += epe * num_frames
        frame_accum += num_frames
    print(f'Normalized AEPE: {epe_accum / frame_accum}')


def write_scene_flows(model, testset, outdir, device):
    """main.py:123-130: frame_%04d.flo of the forward flow of every pair, evaluated one pair at a time"""
    import torch
    from sin_inn_amd.flowdata import writeFlow
    os.makedirs(outdir, exist_ok=True)
    files = []
    with torch.no_grad():
        for i in range(len(testset)):
            f1, _, t, s = testset[i][:4]
            f1, t = f1.to(device).unsqueeze(0), t.to(device).unsqueeze(0)
            flow, _ = model(f1, t, s)
            files.append(path.join(outdir, f'frame_{i + 1:04d}.flo'))
            writeFlow(files[-1], flow.squeeze(0).permute(1, 2, 0).cpu().numpy())
    return files


def sintel_submission(args):
    """main.py:109-130: sintel_submission/<clean | final>/<scene>/frame_%04d.flo for every scene beside --input-video; the pass is
    `clean` if --name ends in it, else `final` (the reference fails on a name that ends in neither).  With --synthetic or
    --layered the one generated scene is written."""
    import torch
    from sin_inn_amd.flowdata import get_video
    from sin_inn_amd.flowtrainer import FlowTrainer
    device = torch.device('cuda', _devices(args)[0])
    sintel_pass = 'clean' if args.name.endswith('clean') else 'final'
    scenes = [None] if args.synthetic or getattr(args, 'layered', None) else sorted(os.listdir(path.dirname(args.input_video)))
    for entry in scenes:
        video, scene = get_video(args.input_video if entry is None else path.join(path.dirname(args.input_video), entry), args)
        args.net = build_net(args)
        model = FlowTrainer.load_from_checkpoint(_latest_ckpt(scene, args.name), args=args)
        model.to(device)
        write_scene_flows(model, video.testset, path.join('sintel_submission', sintel_pass, scene), device)


def main(argv=None):
    args = get_args(argv)
    args.net = build_net(args)
    {'train': train_model, 'test': test_model, 'summarize': summarize_model, 'sintel': sintel_submission}[args.operation](args)


if __name__ == '__main__':
    main()
