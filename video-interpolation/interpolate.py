"""Slow motion from a fitted flow network: the frames between every consecutive pair of a clip, written as PNGs.

    python video-interpolation/interpolate.py --input-video <sintel scene folder> --name NAME --net PRBF --factor 8
    python video-interpolation/interpolate.py --synthetic 4 24 40 --name smoke --net RBF --fit-epochs 2 --factor 3 --out frames
    python video-interpolation/interpolate.py --synthetic 9 24 40 --name smoke --net RBF --fit-epochs 2 --holdout 2
    python video-interpolation/interpolate.py --layered 9 96 160 --name occl --net RBF --fit-epochs 300 --holdout 2 --synthesis gather --occlusion wang

The network is the one `main.py train --name NAME --net NET` fitted to the clip: the newest checkpoint under
checkpoints/<scene>/<NAME> is loaded as `main.py test` loads it (same folder, same tie-break).  For pair i of the clip and
j = 0 .. factor - 1 the frame at tau = j / factor is written to <out>/frame_<i + 1:04d>_<j:02d>.png; j = 0 is the source frame
itself, written from the data, the others come from `FlowTrainer.interpolate` (sin_inn_amd.flowsynth: softmax splatting of both
frames along the pair's two flows, blended; one call per batch of pairs, whatever the factor).  After the last pair the last
source frame is written as frame_<T:04d>_00.png.

  --input-video DIR | --synthetic T H W | --layered T H W   the clip: an `Images` folder, a `SyntheticClip` of T frames of H x W, or a
                   `LayeredClip` of that size (two moving layers: real occlusion)
  --factor F       F - 1 new frames per pair (default 2)
  --size S         --input-video: the shorter side of the frames (default 436)
  --out DIR        where the PNGs go (default results/interp_<scene>_<name>_x<factor>)
  --gif            also results/interp_<scene>_<name>_x<factor>.gif
  --fit-epochs N   train N epochs first through FlowTrainer (default 0: a checkpoint must exist); with it no checkpoint is read
  --holdout S      score the network: keep every S-th frame of the clip (the network is the one fitted with `main.py --holdout S`, or
                   is fitted here on the kept frames), synthesize the S - 1 frames between every kept pair (--factor becomes S) and
                   compare them with the real ones by PSNR and SSIM, on the bytes the PNGs hold.  <out>/quality.jsonl gets one line
                   per held-out frame (pair, j, tau, then psnr, ssim and mse of the network, of the linear blend of the two kept frames
                   and of the nearer kept frame repeated) and a last line with the means, which are also printed as a table
  --synthesis R    splat (default): the network's flows at the pair's time stamp, scaled by tau, softmax-splatted;
                   gather: the network's flows at the in-between time itself, both frames read through a backward warp.
                   The files written and quality.jsonl keep their format; the last line of quality.jsonl names the synthesis
  --back B         --synthesis gather: network (default) takes the flow toward the previous frame from the network at s - dt;
                   reverse uses the negated forward flow at s and evaluates half the time stamps
  --occlusion O    --synthesis gather only: wang or brox, the occlusion-aware gather rule with the trainer's masks of that
                   operator, computed from the network's flows at the frame times; the last line of quality.jsonl names it
"""
import argparse
import importlib.util
import os
import os.path as path
import sys

ROOT = path.dirname(path.dirname(path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def flow_main():
    """main.py of this folder as a module, loaded from its file (the repository root holds a main.py of its own)"""
    spec = importlib.util.spec_from_file_location('flow_main', path.join(path.dirname(path.abspath(__file__)), 'main.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def get_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--input-video', help='an Images scene folder (frame_0001.png ..)')
    src.add_argument('--synthetic', nargs=3, type=int, metavar=('T', 'H', 'W'), help='a SyntheticClip of T frames of H x W')
    src.add_argument('--layered', nargs=3, type=int, metavar=('T', 'H', 'W'), help='a LayeredClip of T frames of H x W (occlusion)')
    ap.add_argument('--name', required=True, help='the run whose newest checkpoint is loaded')
    ap.add_argument('--net', required=True, help='the network of that run (main.py --net)')
    ap.add_argument('--factor', type=int, help='time steps per pair: factor - 1 new frames between two source frames (default 2)')
    ap.add_argument('--size', type=int, default=436, help='--input-video: the shorter side of the frames')
    ap.add_argument('--out', help='folder of the PNGs (default results/interp_<scene>_<name>_x<factor>)')
    ap.add_argument('--gif', action='store_true', help='also write results/interp_<scene>_<name>_x<factor>.gif')
    ap.add_argument('--fit-epochs', type=int, default=0, metavar='N', help='train N epochs first instead of loading a checkpoint')
    ap.add_argument('--batch', type=int, default=1, help='pairs per call')
    ap.add_argument('--holdout', type=int, metavar='S', help='keep every S-th frame and score the synthesis of the others; sets --factor')
    ap.add_argument('--synthesis', choices=('splat', 'gather'), default='splat', help='the synthesis rule (DESIGN 17 / 19)')
    ap.add_argument('--back', choices=('network', 'reverse'), default='network',
                    help='--synthesis gather: where the flow toward the previous frame comes from')
    ap.add_argument('--occlusion', choices=('wang', 'brox'),
                    help='--synthesis gather: the occlusion-aware rule with the masks of this operator (DESIGN 26)')
    ap.add_argument('--loss-between', type=float, default=0, metavar='W',
                    help='--fit-epochs: weight of the in-between consistency loss (main.py --loss-between; DESIGN 22)')
    ap.add_argument('--between-taus', type=int, metavar='K', help='--loss-between: in-between times drawn per step (default 1)')
    ap.add_argument('--between-points', type=int, metavar='N',
                    help='--loss-between: N random points a step instead of whole frames (main.py --between-points; DESIGN 23)')
    ap.add_argument('--between-back', choices=('network', 'reverse'), default='network', help='--loss-between: as --back')
    ap.add_argument('--loss-smooth-at', type=float, default=0, metavar='W',
                    help='--fit-epochs: weight of the smoothness prior on the flow Jacobian at random points (main.py --loss-smooth-at; DESIGN 24)')
    ap.add_argument('--smooth-points', type=int, metavar='N', help='--loss-smooth-at: random points a step (default 4096)')
    return ap


def get_args(argv=None):
    ap = get_parser()
    a = ap.parse_args(argv)
    if a.holdout is not None:
        if a.holdout < 2:
            ap.error('--holdout S: S >= 2 (every S-th frame is kept)')
        if a.factor is not None and a.factor != a.holdout:
            ap.error(f'--factor {a.factor} and --holdout {a.holdout} disagree: --holdout S sets the factor to S')
        a.factor = a.holdout
    elif a.factor is None:
        a.factor = 2
    if a.factor < 1 or a.factor > 65:
        ap.error('--factor: 1 .. 65 (one call synthesizes factor - 1 <= 64 times)')
    if a.occlusion is not None and a.synthesis != 'gather':
        ap.error(f'--occlusion {a.occlusion} is the masked gather rule: it is valid only with --synthesis gather')
    if a.between_points is not None and a.between_taus is not None:
        ap.error('--between-taus draws whole frames, --between-points sampled points: give one of them')
    if a.between_points is not None and a.between_points < 1:
        ap.error('--between-points N: N >= 1')
    if a.fit_epochs < 0 or a.batch < 1:
        ap.error('--fit-epochs >= 0 and --batch >= 1')
    return a


def frame_plan(num_frames, factor):
    """[(file name, pair index, j)] in writing order; j == 0: source frame `pair index`, the last entry the last source frame"""
    plan = [(f'frame_{i + 1:04d}_{j:02d}.png', i, j) for i in range(num_frames - 1) for j in range(factor)]
    plan.append((f'frame_{num_frames:04d}_00.png', num_frames - 1, 0))
    return plan


def trainer_args(a):
    """the namespace of main.py (its defaults for the losses) for this clip, run and network"""
    m = flow_main()
    argv = ['test', '--name', a.name, '--net', a.net, '--size', str(a.size), '--test-size', str(a.size), '--test-batch', str(a.batch),
            '--epochs', str(max(a.fit_epochs, 1))]
    if a.layered:
        argv += ['--layered', *map(str, a.layered)]
    else:
        argv += ['--synthetic', *map(str, a.synthetic)] if a.synthetic else ['--input-video', a.input_video]
    if a.holdout:
        argv += ['--holdout', str(a.holdout)]
    if a.loss_smooth_at and a.fit_epochs:
        argv += ['--loss-smooth-at', str(a.loss_smooth_at)] + (['--smooth-points', str(a.smooth_points)] if a.smooth_points is not None else [])
    if a.loss_between and a.fit_epochs:
        argv += ['--loss-between', str(a.loss_between), '--between-back', a.between_back]
        argv += ['--between-points', str(a.between_points)] if a.between_points is not None else ['--between-taus', str(a.between_taus or 1)]
    args = m.get_args(argv)
    args.net = m.build_net(args)
    return m, args


def load_model(a):
    """(FlowTrainer on the device, data module, scene name): fitted here for --fit-epochs, else from the newest checkpoint"""
    import torch
    from sin_inn_amd.flowdata import get_video
    from sin_inn_amd.flowtrainer import FlowTrainer
    from sin_inn_amd.lightning import Trainer
    m, args = trainer_args(a)
    video, scene = get_video(args.input_video, args)
    device = torch.device('cuda', 0)
    if a.fit_epochs:
        if getattr(args, 'loss_between', 0) != 0:
            args.between_dt = 2 / (len(video.testset.T) - 1)   # the clip being fitted: under --holdout the kept frames
        model = FlowTrainer(args, test_tag=f'{scene}_{a.name}')
        Trainer(gpus=[0], max_epochs=a.fit_epochs, check_val_every_n_epoch=a.fit_epochs + 1).fit(model, video)
    else:
        model = FlowTrainer.load_from_checkpoint(m._latest_ckpt(scene, a.name), args=args, test_tag=f'{scene}_{a.name}')
    return model.to(device), video, scene


def _to_device(batch, device):
    import torch
    return [t.to(device) if torch.is_tensor(t) else t for t in batch]


METHODS = ('net', 'blend', 'repeat')


def quality_records(scores, first):
    """one record per held-out frame of a batch: `scores` is `FlowTrainer.holdout_quality`'s dict of (n, K) results, `first` the
    index of the batch's first pair"""
    host = {m: (scores[m].psnr.cpu().tolist(), scores[m].ssim.cpu().tolist(), scores[m].mse.cpu().tolist()) for m in METHODS}
    n, k = len(host['net'][0]), len(host['net'][0][0])
    records = []
    for i in range(n):
        for j in range(k):
            rec = {'pair': first + i, 'j': j + 1, 'tau': (j + 1) / (k + 1)}
            for m in METHODS:
                rec[f'psnr_{m}'], rec[f'ssim_{m}'], rec[f'mse_{m}'] = host[m][0][i][j], host[m][1][i][j], host[m][2][i][j]
            records.append(rec)
    return records


def quality_means(records):
    """the last line of quality.jsonl: the means over the held-out frames (an infinite PSNR makes its mean infinite)"""
    out = {'mean': True, 'frames': len(records)}
    for m in METHODS:
        for what in ('psnr', 'ssim', 'mse'):
            out[f'{what}_{m}'] = sum(r[f'{what}_{m}'] for r in records) / len(records)
    return out


def quality_table(means):
    names = {'net': 'network', 'blend': 'linear blend', 'repeat': 'nearer frame'}
    lines = [f'{"":14s}{"PSNR / dB":>10s}{"SSIM":>9s}']
    lines += [f'{names[m]:14s}{means["psnr_" + m]:10.3f}{means["ssim_" + m]:9.5f}' for m in METHODS]
    return '\n'.join(lines)


def main(argv=None):
    a = get_args(argv)
    import json
    import numpy as np
    import torch
    from PIL import Image
    from sin_inn_amd.flowtrainer import save_gif
    model, video, scene = load_model(a)
    device = next(model.parameters()).device
    clip = video.testset.video                                    # (T, 3, h, w) in [0, 1], on the host
    num_frames = clip.shape[0]
    tag = f'interp_{scene}_{a.name}_x{a.factor}'
    out_dir = a.out or path.join('results', tag)
    os.makedirs(out_dir, exist_ok=True)
    taus = [j / a.factor for j in range(1, a.factor)]
    source = (clip * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).numpy()         # (T, h, w, 3)
    how = {}
    if a.synthesis == 'gather':
        how = dict(synthesis='gather', dt=2 / (num_frames - 1), back=a.back)        # the clip fitted: under --holdout the kept frames
        if a.occlusion:
            how['occlusion'] = a.occlusion
    between = {}                                                   # (pair, j) -> (h, w, 3) bytes
    records = []
    if taus:
        first = 0
        for batch in video.test_dataloader():
            batch = _to_device(batch, device)
            frames, u8 = model.interpolate(batch, taus, u8=True, **how)
            if a.holdout:
                held = torch.stack([video.testset.held(first + n)[0] for n in range(batch[0].shape[0])])
                records += quality_records(model.holdout_quality(batch, held, taus, frames=frames), first)
            u8 = u8.permute(0, 1, 3, 4, 2).cpu().numpy()           # (n, K, h, w, 3)
            for n in range(u8.shape[0]):
                for j in range(1, a.factor):
                    between[(first + n, j)] = u8[n, j - 1]
            first += u8.shape[0]
    written = []
    for name, i, j in frame_plan(num_frames, a.factor):
        img = source[i] if j == 0 else between[(i, j)]
        Image.fromarray(np.ascontiguousarray(img)).save(path.join(out_dir, name))
        written.append(img)
    if a.gif:
        os.makedirs('results', exist_ok=True)
        save_gif(path.join('results', f'{tag}.gif'), np.stack(written), fps=4 * a.factor)
    if a.holdout:
        means = quality_means(records)
        means['synthesis'] = a.synthesis if a.synthesis == 'splat' else f'gather/{a.back}' + (f'/{a.occlusion}' if a.occlusion else '')
        with open(path.join(out_dir, 'quality.jsonl'), 'w') as f:
            for rec in records + [means]:
                f.write(json.dumps(rec) + '\n')
        print(quality_table(means))
    print(f'{len(written)} frames of {clip.shape[-2]} x {clip.shape[-1]} in {out_dir} ({num_frames} source frames, x{a.factor})')


if __name__ == '__main__':
    main()
