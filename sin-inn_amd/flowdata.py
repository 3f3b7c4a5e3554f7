"""The data side of the flow trainer: Middlebury .flo files, a folder of frames with ground-truth flow (Sintel's layout), a synthetic
clip with analytic ground truth, and the data module that hands them to the trainer.

    readFlow / writeFlow       video-interpolation/my_utils/utils.py:27-77
    BaseMedia / Images         video-interpolation/data.py:10-18, 67-89
    LightningLoader / get_video   video-interpolation/data.py:92-119   (num_workers=0: the clips are resident tensors)
    SyntheticClip              this project's; generalises tools/fit_flow.make_pair to a clip
    LayeredClip                this project's; two textured layers with constant velocities: real occlusion, analytic flows and masks
    Holdout                    this project's; every step-th frame of a clip, the frames between them kept back for scoring

Everything here runs on the host; the trainer moves batches to the device.

Unpinned: the resize.  The reference resizes with torchvision's `T.Resize(size, antialias=True)` on a tensor, which calls
`torch.nn.functional.interpolate(mode='bilinear', antialias=True, align_corners=False)` with the shorter side set to `size` and
the longer one to `int(size * long / short)`.  torchvision is not installed here, so `Images` makes that interpolate call itself
and no fixture compares the two.

Out of scope: `VideoClip` (imageio decoding + RAFT flows, data.py:21-64).
"""
import math
import os
import os.path as path

import numpy as np
import torch
import torch.utils.data as data

from .lightning import LightningDataModule

FLO_MAGIC = 202021.25


def readFlow(fn):
    """utils.py:27-47: (h, w, 2) float32 array of a Middlebury .flo file (float32 magic 202021.25, int32 w, int32 h, interleaved
    u, v rows; little-endian); None, with a message, if the magic is wrong."""
    with open(fn, 'rb') as f:
        magic = np.fromfile(f, np.float32, count=1)
        if magic.size != 1 or magic[0] != np.float32(FLO_MAGIC):
            print('Magic number incorrect. Invalid .flo file')
            return None
        w = int(np.fromfile(f, np.int32, count=1)[0])
        h = int(np.fromfile(f, np.int32, count=1)[0])
        values = np.fromfile(f, np.float32, count=2 * w * h)
        return np.resize(values, (h, w, 2))


def writeFlow(filename, uv, v=None):
    """utils.py:49-77: `uv` (h, w, 2), or u and v as two (h, w) arrays."""
    if v is None:
        assert uv.ndim == 3 and uv.shape[2] == 2
        u, v = uv[:, :, 0], uv[:, :, 1]
    else:
        u = uv
    assert u.shape == v.shape
    height, width = u.shape
    with open(filename, 'wb') as f:
        np.array([FLO_MAGIC], np.float32).tofile(f)
        np.array(width).astype(np.int32).tofile(f)
        np.array(height).astype(np.int32).tofile(f)
        np.stack((u, v), axis=2).astype(np.float32).tofile(f)


class BaseMedia(data.Dataset):
    """data.py:10-18: item i is the pair (frame i, frame i + 1) with the time of frame i."""

    def __len__(self):
        return self.video.size(0) - 1

    def __getitem__(self, index):
        if self.gt_available:
            return self.video[index], self.video[index + 1], self.T[index], self.flow_scale, self.flow[index]
        return self.video[index], self.video[index + 1], self.T[index], self.flow_scale


def resize_shorter_side(x, size):
    """(c, h, w) -> shorter side `size`, longer side int(size * long / short): torchvision's tensor Resize(size, antialias=True)"""
    h, w = x.shape[-2:]
    short, long = (h, w) if h <= w else (w, h)
    new_short, new_long = size, int(size * long / short)
    new_hw = (new_short, new_long) if h <= w else (new_long, new_short)
    if new_hw == (h, w):
        return x
    return torch.nn.functional.interpolate(x[None], size=new_hw, mode='bilinear', antialias=True, align_corners=False)[0]


def _read_frame(fn):
    """PIL image -> (c, h, w) float in [0, 1] (torchvision's ToTensor for 8-bit images)"""
    from PIL import Image
    with Image.open(fn) as im:
        a = np.asarray(im)
    assert a.dtype == np.uint8, f'{fn}: 8-bit frames expected'
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(torch.float32) / 255


class Images(BaseMedia):
    """data.py:67-89: `root` holds frame_0001.png, frame_0002.png, ... and nothing else; ground truth, if there is any, is
    root/../../flow/<scene>/frame_%04d.flo, resized like the frames and multiplied by size / h so that it stays in pixels."""

    def __init__(self, root, size=200):
        super().__init__()
        from PIL import Image
        num_frames = len(os.listdir(root))
        frames = [path.join(root, f'frame_{i + 1:04d}.png') for i in range(num_frames)]
        with Image.open(frames[0]) as im:
            w, h = im.size
        assert h <= w, 'Frame should be landscape oriented'
        self.video = torch.stack([resize_shorter_side(_read_frame(f), size) for f in frames])
        self.T = torch.linspace(-1, 1, self.video.size(0))

        scene, _ = path.splitext(path.basename(root))
        flow_dir = path.join(root, '../../flow')
        if path.isdir(flow_dir):
            self.gt_available = True
            rescale_ratio = size / h
            flows = [readFlow(path.join(flow_dir, scene, f'frame_{i + 1:04d}.flo')) for i in range(num_frames - 1)]
            self.flow = torch.stack([resize_shorter_side(torch.tensor(f).permute(2, 0, 1), size) for f in flows]) * rescale_ratio
        else:
            self.gt_available = False
        self.flow_scale = self.video.shape[-1] / 5


def texture(x, y, gen_seed):
    """3-channel sum of 12 low-frequency plane waves per channel, values in about [0, 1]; x, y in pixels (any shape).  The texture
    of tools/fit_flow.py: the same seed gives the same image."""
    g = torch.Generator().manual_seed(gen_seed)
    k = (torch.rand(3, 12, 2, generator=g) - 0.5) * 0.6          # radians per pixel
    ph = torch.rand(3, 12, generator=g) * 2 * math.pi
    k, ph = k.to(x), ph.to(x)
    arg = k[:, :, 0, None, None] * x[None, None] + k[:, :, 1, None, None] * y[None, None] + ph[:, :, None, None]
    return 0.5 + torch.sin(arg).mean(1) * 1.2


class SyntheticClip(BaseMedia):
    """`frames` frames of h x w with analytic ground-truth flow, the interface of `Images`.

    frame_i(x) = texture(x - s_i d(x)),  s_i = i / (frames - 1),  d = (u, v) the smooth displacement of tools/fit_flow.make_pair:
    the displacement grows linearly with time and frames 0 and `frames - 1` are make_pair's pair (evaluated in float64 here, so equal to fp32 rounding).  The
    ground truth of pair i is the flow that carries frame i onto frame i + 1: the point x of frame i shows the texture at
    p = x - s_i d(x), and frame i + 1 shows that texture at the y with y - s_{i+1} d(y) = p, so flow_i(x) = y - x.  y is the fixed
    point of y -> p + s_{i+1} d(y), a contraction because |grad d| < 1 (asserted), iterated in float64 to convergence."""

    def __init__(self, frames, h, w, seed=0):
        super().__init__()
        assert frames >= 2 and h >= 8 and w >= 8, 'SyntheticClip: at least 2 frames of 8 x 8'
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')

        def disp(x, y):
            return 1.5 * torch.sin(y / h * math.pi) + 0.5, 1.0 * torch.cos(x / w * math.pi)

        assert 1.5 * math.pi / h < 0.9 and math.pi / w < 0.9
        s = [i / (frames - 1) for i in range(frames)]
        u, v = disp(xx, yy)
        self.video = torch.stack([texture(xx - si * u, yy - si * v, seed) for si in s]).to(torch.float32)
        flows = []
        for i in range(frames - 1):
            px, py = xx - s[i] * u, yy - s[i] * v
            x1, y1 = xx.clone(), yy.clone()
            for _ in range(200):
                du, dv = disp(x1, y1)
                nx, ny = px + s[i + 1] * du, py + s[i + 1] * dv
                delta = max(float((nx - x1).abs().max()), float((ny - y1).abs().max()))
                x1, y1 = nx, ny
                if delta < 1e-13:
                    break
            flows.append(torch.stack((x1 - xx, y1 - yy)))
        self.flow = torch.stack(flows).to(torch.float32)
        self.T = torch.linspace(-1, 1, frames)
        self.gt_available = True
        self.flow_scale = w / 5


class LayeredClip(BaseMedia):
    """`frames` frames of h x w with real occlusion and analytic ground truth, the interface of `Images`: two layers
    with constant velocities `bg`, `fg` = (vx, vy) in pixels per frame.

    The background is the plane texture(.., seed) and fills the frame; the foreground is an axis-aligned rectangle of
    (h // 3) x (w // 3) pixels textured with texture(.., seed + 1), placed so that it stays inside the frame for the whole clip (in the
    middle of the positions that allow it, on a half-integer corner).  Its edge is hard: at the frame time s -- any real number, the
    frames of `video` sit at s = 0 .. frames - 1 -- the pixel (x, y) shows the foreground where its centre lies inside the rectangle,
    x0 + s vx <= x < x0 + s vx + rw and likewise in y, and the background elsewhere.  Each layer shows its texture at the pixel's
    position minus s times the layer's velocity.  Everything is evaluated in float64; `video` and `flow` are its fp32 roundings.

        frame_at(s)             the frame at time s, (3, h, w) float64;  sample_at(s, x, y): the same content at any coordinates
        flow_between(s, s2)     (2, h, w) float64 on the grid at s: the velocity of the layer each pixel shows, times s2 - s
        visible(i, j)           (h, w) bool: the pixels of the frame at i whose surface the frame at j still shows -- every foreground
                                pixel, and a background pixel unless the rectangle covers its position at time j.  Leaving the
                                frame is not counted: a sampler sees that from its taps

    `flow[i]` is flow_between(i, i + 1), the ground truth of pair i."""

    def __init__(self, frames, h, w, seed=0, bg=(3.0, 0.0), fg=(-2.0, 1.5)):
        super().__init__()
        assert frames >= 2 and h >= 8 and w >= 8, 'LayeredClip: at least 2 frames of 8 x 8'
        self.h, self.w, self.seed = h, w, seed
        self.bg, self.fg = (float(bg[0]), float(bg[1])), (float(fg[0]), float(fg[1]))
        self.rh, self.rw = h // 3, w // 3
        last = frames - 1

        def start(size, length, v):
            lo, hi = -min(0.0, last * v), size - length - max(0.0, last * v)      # the corner positions that keep the rectangle inside
            if lo > hi:
                raise ValueError(f'LayeredClip: a foreground of {length} pixels moving {v} a frame leaves a frame of {size} within '
                                 f'{frames} frames')
            return min(max(math.floor((lo + hi) / 2) + 0.5, lo), hi)

        self.x0, self.y0 = start(w, self.rw, self.fg[0]), start(h, self.rh, self.fg[1])
        self.yy, self.xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
        self.video = torch.stack([self.frame_at(i) for i in range(frames)]).to(torch.float32)
        self.flow = torch.stack([self.flow_between(i, i + 1) for i in range(frames - 1)]).to(torch.float32)
        self.T = torch.linspace(-1, 1, frames)
        self.gt_available = True
        self.flow_scale = w / 5

    def covered(self, s, x, y):
        """where the rectangle at time s covers the points (x, y) (float64, any shape)"""
        left, top = self.x0 + s * self.fg[0], self.y0 + s * self.fg[1]
        return (x >= left) & (x < left + self.rw) & (y >= top) & (y < top + self.rh)

    def sample_at(self, s, x, y):
        """the clip's content at time s at the points (x, y), two-dimensional float64 tensors of any values: (3, ..) float64"""
        back = texture(x - s * self.bg[0], y - s * self.bg[1], self.seed)
        front = texture(x - s * self.fg[0], y - s * self.fg[1], self.seed + 1)
        return torch.where(self.covered(s, x, y)[None], front, back)

    def frame_at(self, s):
        return self.sample_at(float(s), self.xx, self.yy)

    def flow_between(self, s, s2):
        front = self.covered(float(s), self.xx, self.yy)
        vx = torch.where(front, torch.full_like(self.xx, self.fg[0]), torch.full_like(self.xx, self.bg[0]))
        vy = torch.where(front, torch.full_like(self.xx, self.fg[1]), torch.full_like(self.xx, self.bg[1]))
        return torch.stack((vx, vy)) * (float(s2) - float(s))

    def visible(self, i, j):
        i, j = float(i), float(j)
        back = ~self.covered(i, self.xx, self.yy)
        return ~(back & self.covered(j, self.xx + (j - i) * self.bg[0], self.yy + (j - i) * self.bg[1]))


class Holdout(BaseMedia):
    """Every `step`-th frame of `base` (an `Images` or a `SyntheticClip`) as a clip of its own, the frames between them held out: fit
    on this, synthesize the held-out frames, compare them with the real ones (`FlowTrainer.holdout_quality`).

    The kept frames are base.video[::step], kept = (len - 1) // step + 1 of them, at the times linspace(-1, 1, kept); item i is the
    pair (kept i, kept i + 1) as in `BaseMedia`, with the base's `flow_scale` and no ground-truth flow (`gt_available = False`: the
    base's flows join neighbouring frames, not kept ones).  `held(i)` is the `step - 1` real frames between the two and the times
    tau_j = j / step at which they sit.  The (len - 1) % step frames after the last kept one are dropped (`dropped`)."""

    def __init__(self, base, step):
        super().__init__()
        step = int(step)
        if step < 2:
            raise ValueError(f'Holdout: step = {step}; at least every 2nd frame is kept')
        frames = base.video.size(0)
        if frames < step + 1:
            raise ValueError(f'Holdout: a clip of {frames} frames is too short for step {step}: it needs at least {step + 1}')
        self.base, self.step = base, step
        self.kept_indices = list(range(0, frames, step))
        self.dropped = (frames - 1) % step
        self.video = base.video[::step]
        self.T = torch.linspace(-1, 1, self.video.size(0))
        self.flow_scale = base.flow_scale
        self.gt_available = False

    def held(self, i):
        """(frames (step - 1, C, H, W), taus (step - 1,)) between kept frames i and i + 1"""
        if not 0 <= i < len(self):
            raise IndexError(f'Holdout.held: pair {i} of {len(self)}')
        first = self.kept_indices[i]
        taus = torch.arange(1, self.step, dtype=torch.float32) / self.step
        return self.base.video[first + 1:first + self.step], taus

    def with_held(self):
        """the data set the validation step reads: item i = (kept i, kept i + 1, time, flow scale, held frames, taus)"""
        return _HoldoutPairs(self)


class _HoldoutPairs(data.Dataset):
    def __init__(self, holdout):
        self.holdout = holdout

    def __len__(self):
        return len(self.holdout)

    def __getitem__(self, index):
        return tuple(self.holdout[index]) + tuple(self.holdout.held(index))


class LightningLoader(LightningDataModule):
    """data.py:92-104, with num_workers=0."""

    def __init__(self, trainset, testset, train_batch, test_batch):
        super().__init__()
        self.trainset = trainset
        self.testset = testset
        self.train_batch = train_batch
        self.test_batch = test_batch

    def train_dataloader(self):
        return data.DataLoader(self.trainset, batch_size=self.train_batch, num_workers=0, shuffle=True)

    def val_dataloader(self):
        return data.DataLoader(self.testset, batch_size=self.test_batch, num_workers=0)

    def test_dataloader(self):
        return data.DataLoader(self.testset, batch_size=self.test_batch, num_workers=0)


class HoldoutLoader(LightningLoader):
    """LightningLoader over two `Holdout` sets: training and testing see the kept pairs, validation also the held-out frames"""

    def val_dataloader(self):
        return data.DataLoader(self.testset.with_held(), batch_size=self.test_batch, num_workers=0)


def get_video(input_video, args):
    """data.py:107-119: (data module, scene name).  `args.synthetic = (frames, h, w)` selects a SyntheticClip, scene 'synthetic',
    `args.layered = (frames, h, w)` a LayeredClip, scene 'layered'; a file (the reference's VideoClip) is refused.  `args.holdout = S` (main.py --holdout) wraps both sets in `Holdout(.., S)`."""
    synthetic, layered = getattr(args, 'synthetic', None), getattr(args, 'layered', None)
    if synthetic:
        frames, h, w = synthetic
        trainset = testset = SyntheticClip(frames, h, w)
        scene = 'synthetic'
    elif layered:
        frames, h, w = layered
        trainset = testset = LayeredClip(frames, h, w)
        scene = 'layered'
    elif path.isdir(input_video):
        trainset = Images(input_video, size=args.size)
        testset = Images(input_video, size=args.test_size)
        scene, _ = path.splitext(path.basename(input_video))
    else:
        raise NotImplementedError(f'{input_video}: not a folder of frames; video files (VideoClip: imageio + RAFT) are out of scope')
    if trainset.gt_available:
        print(f'Max flow: {trainset.flow.max().item()}, estimated scale: {trainset.flow_scale}')
    holdout = getattr(args, 'holdout', None)
    if holdout:
        trainset = Holdout(trainset, holdout)
        testset = trainset if testset is trainset.base else Holdout(testset, holdout)
        print(f'Holdout: every {holdout}. frame kept, {len(trainset.kept_indices)} of {trainset.base.video.size(0)}; '
              f'{trainset.dropped} trailing frames dropped')
        return HoldoutLoader(trainset, testset, args.batch, args.test_batch), scene
    return LightningLoader(trainset, testset, args.batch, args.test_batch), scene
