"""FlowTrainer, the training / validation / test step of the flow path (video-interpolation/trainer.py:15-135), on this project's
kernels: the flow-field network (`flownet.flow_fields`), the photometric losses (`flowloss`), the Resample2d warp
(`functional.flow_warp_l1`), FusedLAMB, and the operators of csrc/flowtrain.hip that take the place of chains of small torch
launches on strided views (the end-point error, `mask * (splat != 0)`), of a per-frame trip to the host (flow2img) and of the
(N, 8) index and weight tensors of a spatial controller's loss log (error_stash).

    flow_epe / splat_mask / flow2img / make_color_wheel   trainer.py:58, 64, 68; my_utils/flow_viz.py:6-127
    error_stash / error_stash_composed / error_map        the per-point loss of the step and its stash
    FlowTrainer                                            trainer.py:15-135

Under a StashedSpatialController (`main.py --spatially-adaptive`) the step needs a loss PER POINT.  The reference defines none: its
trainer hands the controller the scalar and fails with an IndexError, and it never calls `update_progress`.  Here it is the integrand
of the two L1 terms at the target pixel, E = 0.5 (mean_c |m1 S1 - m1 I1| + mean_c |m2 S2 - m2 I2|); `training_step` keeps the six
tensors, `on_after_backward` (the controller updates its grid in place, so not before the backward pass) stashes them and runs
`update_progress()` every `block_iterations` steps.

The step makes no host round trip of its own.  The two it inherits: `LinearControllerEarly.stash_iteration` reads the loss
(progressive networks only, as in the reference), and the flow scale of a batch is read once per frame size (it is a constant of
the data set, `W / 5`) and cached.

Differences from the reference, all on purpose:
  * `train/PSNR` is not logged.  The reference logs torchmetrics' `PSNR()` with no data range, which infers the range from the
    targets it has seen so far; torchmetrics is not installed here and that running range cannot be pinned.
  * `train/loss_epoch` is logged beside `train/loss`: the mean over the epoch so far (what Lightning's `on_epoch=True` records).
  * `train/ssim` is logged whenever `--loss-ssim` is non-zero; the reference tests the loss VALUE, which reads it back.
  * wandb is replaced by the FileLogger of `sin_inn_amd.lightning`; the flow and occlusion videos are always written as GIFs under
    results/ (with PIL; the reference uses imageio, and only when there is no logger), and the test EPE is printed and logged as
    `test/EPE`.
  * on resume the controller of a progressive network gets its `iteration`, `cur_block` and `next_block` back (`on_load_checkpoint`);
    the reference restores the mask alone and restarts the schedule.
  * `--loss-between W` adds a photometric consistency term at random in-between times, which the reference has not:
    the virtual frame at s = t0 + tau dt is read once from frame 1 alone and once from frame 2 alone through `flowsynth.gather`
    (blend weights 0 and 1), and W mean |A - B| trains the flows at s through the operator's gradient.  Off (W = 0) the step is
    the reference's, launch for launch.  `--between-points N` draws the term at N random (pair, tau, y, x) a step
    instead of whole frames: the network runs on N or 2 N points through `flownet.flow_at` and `flowsynth.gather_at` reads the
    two frames at them.
"""
import ctypes as C
import os
import random

import numpy as np
import torch

from . import _lib, flowcaps, flowloss as FL, flownet
from .functional import flow_warp_l1
from .lightning import LightningModule, load_checkpoint
from .ops import _stream, ptr
from .optim import FusedLAMB

check = _lib.check


def make_color_wheel():
    """flow_viz.py:80-127: the Middlebury colour wheel, 55 x 3 float64 in 0..255.  Six segments (RY, YG, GC, CB, BM, MR) of 15, 6,
    4, 11, 13 and 6 colours; within a segment one channel stays at 255 while another ramps up as floor(255 i / len) or down as
    255 - floor(255 i / len)."""
    segments = ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True), (6, 0, 2, False))
    wheel = np.zeros((sum(s[0] for s in segments), 3))
    row = 0
    for length, full, ramp, rising in segments:
        steps = np.floor(255 * np.arange(length) / length)
        wheel[row:row + length, full] = 255
        wheel[row:row + length, ramp] = steps if rising else 255 - steps
        row += length
    return wheel


_WHEELS = {}


def _wheel(device):
    if device not in _WHEELS:
        _WHEELS[device] = torch.from_numpy(make_color_wheel()).to(device)
    return _WHEELS[device]


def _gpu32(t):
    if not t.is_cuda:
        raise NotImplementedError('sin-inn_amd flow-trainer operators run on the GPU only (got a CPU tensor)')
    assert t.dtype == torch.float32, 'fp32 tensors expected'
    return t


def flow_epe(flow, gt, partials=None):
    """mean over (n, y, x) of |flow - gt|_2 (trainer.py:58, 97, 110) as a 0-d device tensor.  `flow` (n, 2, h, w) may be a channel
    slice of the (n, 4, h, w) tensor `flow_fields` returns: it is read in place through its sample stride.  `partials`: optional
    float64 device buffer of at least `sininn_flow_epe_partials(n, h, w)` values (allocated here otherwise; needs no
    initialisation)."""
    flow, gt = _gpu32(flow.detach()), _gpu32(gt.detach()).contiguous()
    n, two, h, w = flow.shape
    assert two == 2 and gt.shape == flow.shape, 'flow_epe expects two (n, 2, h, w) tensors'
    if flow.stride()[1:] != (h * w, w, 1) or flow.stride(0) < 2 * h * w:
        flow = flow.contiguous()
    need = _lib.lib().sininn_flow_epe_partials(n, h, w)
    if partials is None:
        partials = torch.empty(max(need, 1), device=flow.device, dtype=torch.float64)
    assert partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous()
    out = torch.empty(1, device=flow.device, dtype=torch.float32)
    check(_lib.lib().sininn_flow_epe(ptr(flow), flow.stride(0), ptr(gt), n, h, w, C.c_void_p(partials.data_ptr()), partials.numel(),
                                     ptr(out), _stream()))
    return out[0]


GRID_POINTS = 1 << 22          # the most points (t h w) one flow_fields call takes (csrc/flownet_tile.h)


def splat_mask(mask, splat):
    """mask * (splat != 0) (trainer.py:64, 68): `splat` (n, 3, h, w), `mask` (n, 1, h, w) or (n, 3, h, w), float or bool.  No
    gradient, as in the reference (the comparison cuts the graph and the occlusion masks carry none)."""
    splat = _gpu32(splat.detach()).contiguous()
    mask = _gpu32(mask.detach().to(torch.float32)).contiguous()
    n, c, h, w = splat.shape
    assert mask.dim() == 4 and mask.shape[0] == n and tuple(mask.shape[2:]) == (h, w), 'splat_mask: mask and splat disagree'
    out = torch.empty_like(splat)
    check(_lib.lib().sininn_splat_mask(ptr(mask), mask.shape[1], ptr(splat), n, c, h, w, ptr(out), _stream()))
    return out


def flow2img(flow, clip=10):
    """flow_viz.py:6-32 for a batch: (n, 2, h, w) fp32 on the device -> (n, 3, h, w) uint8 on the device; a single (2, h, w) flow
    gives (3, h, w).  Each frame is normalised by its own maximum radius."""
    single = flow.dim() == 3
    flow = _gpu32(flow.detach())
    flow = (flow[None] if single else flow).contiguous()
    n, two, h, w = flow.shape
    assert two == 2, 'flow2img expects (n, 2, h, w)'
    wheel = _wheel(flow.device)
    ws = torch.empty(max(_lib.lib().sininn_flow2img_workspace_floats(n, h, w), 1), device=flow.device, dtype=torch.float32)
    img = torch.empty((n, 3, h, w), device=flow.device, dtype=torch.uint8)
    check(_lib.lib().sininn_flow2img(ptr(flow), n, h, w, float(clip), C.c_void_p(wheel.data_ptr()), wheel.shape[0], ptr(ws),
                                     ws.numel(), C.c_void_p(img.data_ptr()), _stream()))
    return img[0] if single else img


def error_map(softmax1, frame1, mask1, softmax2, frame2, mask2):
    """E (B, H, W) with torch ops: 0.5 (mean_c |m1 S1 - m1 I1| + mean_c |m2 S2 - m2 I2|), the integrand of the two L1 terms of the step
    at every target pixel.  The composed partner of `error_stash(.., error_out=)`."""
    e1 = (mask1 * softmax1 - mask1 * frame1).abs().mean(1)
    e2 = (mask2 * softmax2 - mask2 * frame2).abs().mean(1)
    return 0.5 * (e1 + e2)


def _stash_inputs(tensors):
    out = [_gpu32(t.detach().to(torch.float32) if t.dtype == torch.bool else t.detach()).contiguous() for t in tensors]
    s1, i1, m1, s2, i2, m2 = out
    b, c, h, w = s1.shape
    assert i1.shape == s1.shape and s2.shape == s1.shape and i2.shape == s1.shape, 'error_stash: splats and frames of one shape (B, C, H, W)'
    for m in (m1, m2):
        assert m.dim() == 4 and m.shape[0] == b and tuple(m.shape[2:]) == (h, w), 'error_stash: mask and frames disagree'
    if m1.shape[1] != m2.shape[1]:                             # one channel count per call: widen the narrower mask
        m1, m2 = (m.expand(b, c, h, w).contiguous() for m in (m1, m2))
    return s1, i1, m1, s2, i2, m2


def error_stash(softmax1, frame1, mask1, softmax2, frame2, mask2, times, ys, xs, res, centre_scale, log_buffer, log_counter, *,
                error_out=None, workspace=None):
    """The per-point loss of the unsupervised step, stashed into the loss log of a spatially adaptive controller:

        E[b][y][x]         = 0.5 (mean_c |m1 S1 - m1 I1| + mean_c |m2 S2 - m2 I2|)
        log_buffer[cell]  += sum of alpha(p, k) E[p] over the points p = (times[b], ys[y], xs[x]) and their corners k in `cell`
        log_counter[cell] += the same sum of alpha(p, k)

    with the cells and weights of `StashedSpatialController.cells` (`res` cells per axis, `centre_scale` the six floats of
    `centre_scale_host()`).  softmax*, frame*: (B, C, H, W); mask*: (B, 1 or C, H, W), the masks after `splat_mask`; times (B,), ys (H,),
    xs (W,) on the device.  The two logs (res^3 fp32, device) are updated in place and returned.  Three launches, no atomics, a fixed
    order of summation: equal inputs give equal bits.  `error_out`: an optional (B, H, W) tensor that receives E; `workspace`: an
    optional fp32 device buffer of `sininn_flow_error_stash_workspace_floats(B, H, W, res)` values.  No gradient."""
    s1, i1, m1, s2, i2, m2 = _stash_inputs((softmax1, frame1, mask1, softmax2, frame2, mask2))
    b, c, h, w = s1.shape
    times, ys, xs = (_gpu32(t.detach()).contiguous() for t in (times, ys, xs))
    assert (times.numel(), ys.numel(), xs.numel()) == (b, h, w), 'error_stash: one time per frame, one coordinate per row and column'
    cells = int(res) ** 3
    for log in (log_buffer, log_counter):
        _gpu32(log)
        assert log.is_contiguous() and log.numel() == cells, 'error_stash: the logs hold res^3 values'
    if error_out is not None:
        assert _gpu32(error_out).is_contiguous() and tuple(error_out.shape) == (b, h, w), 'error_out: a contiguous (B, H, W) tensor'
    need = _lib.lib().sininn_flow_error_stash_workspace_floats(b, h, w, int(res))
    if workspace is None:
        workspace = torch.empty(max(need, 1), device=s1.device, dtype=torch.float32)
    assert _gpu32(workspace).is_contiguous()
    check(_lib.lib().sininn_flow_error_stash(ptr(s1), ptr(i1), ptr(m1), ptr(s2), ptr(i2), ptr(m2), m1.shape[1], b, c, h, w, ptr(times),
                                             ptr(ys), ptr(xs), int(res), *(float(v) for v in centre_scale), ptr(log_buffer),
                                             ptr(log_counter), ptr(error_out), ptr(workspace), workspace.numel(), _stream()))
    return log_buffer, log_counter


def error_stash_composed(softmax1, frame1, mask1, softmax2, frame2, mask2, times, ys, xs, cells, log_buffer, log_counter, *,
                         error_out=None):
    """`error_stash` with torch ops, its A / B partner: `error_map`, the flat list of the grid's points, `cells(points)` (a
    StashedSpatialController's: the (N, 8) indices and weights) and two `index_add_`.  A sum, like the fused form, where
    `stash_iteration`'s indexed `+=` keeps one write per repeated index; its order is whatever index_add_ makes it."""
    with torch.no_grad():
        e = error_map(*_stash_inputs((softmax1, frame1, mask1, softmax2, frame2, mask2)))
        gt, gh, gw = torch.meshgrid(times, ys, xs, indexing='ij')
        inds, alphas = cells(torch.stack((gt, gh, gw), dim=-1).view(-1, 3))
        log_buffer.index_add_(0, inds.flatten(), (e.reshape(-1, 1) * alphas).flatten())
        log_counter.index_add_(0, inds.flatten(), alphas.flatten())
        if error_out is not None:
            error_out.copy_(e)
    return log_buffer, log_counter


def save_gif(filename, frames, fps=4):
    """(n, h, w, c) uint8, c = 1 or 3 -> an animated GIF (imageio.mimsave(..., format='GIF', fps=4) in the reference)"""
    from PIL import Image
    frames = np.asarray(frames)
    images = [Image.fromarray(f[:, :, 0] if f.shape[2] == 1 else f) for f in frames]
    images[0].save(filename, format='GIF', save_all=True, append_images=images[1:], duration=int(1000 / fps), loop=0)


class FlowTrainer(LightningModule):
    """trainer.py:15-135.  `args` is the namespace of video-interpolation/main.py with `args.net` the network (a model of
    `sin_inn_amd.flownet` or a controller of `sin_inn_amd.progressive` around one)."""

    def __init__(self, args, test_tag=None):
        super().__init__()
        self.args = args
        self.net = args.net
        self.lr = self.args.lr

        self.occlusion = None
        if args.occl == 'brox':
            self.occlusion = FL.occlusion_brox
        elif args.occl == 'wang':
            self.occlusion = FL.occlusion_wang
        self.l1 = FL.L1Loss(args.loss_l1)
        self.census = FL.CensusLoss(args.loss_census, max_distance=args.census_width)
        self.ssim = FL.SSIMLoss(args.loss_ssim)
        self.smooth1 = FL.BilateralSmooth(args.loss_smooth1, args.edge_func, args.edge_constant, 1)

        self.test_tag = test_tag
        self.completed_training = False
        self.hparams = {k: v for k, v in vars(args).items() if k != 'net'}
        self._scales = {}
        self._ones = {}
        self._epoch_means = {}
        self.fused = True                    # False: the torch expressions of the flowtrain operators (tools/bench_flowtrainer.py)
        self._stash = None                   # spatial controller: the six tensors of this step's per-point loss, until on_after_backward
        # the in-between consistency loss: off unless the namespace carries a non-zero weight
        self.between_weight = float(getattr(args, 'loss_between', 0) or 0)
        self.between_rng = None
        self.between_points = None
        if self.between_weight != 0 and int(self.net.domain_dim) != 3:
            raise ValueError(f'domain_dim {int(self.net.domain_dim)}: --loss-between evaluates the network at times between two frames; a '
                             'network on (y, x) has no time axis')
        # the options' own rules are the command line's (flowcaps); the network's Jacobian before the range of --smooth-points, as ever
        flowcaps.check_step_options(args, GRID_POINTS, lambda: flownet._refuse_jacobian(self.net, what='--loss-smooth-at'))
        if self.between_weight != 0:
            self.between_taus = int(getattr(args, 'between_taus', 1))
            self.between_back = getattr(args, 'between_back', 'network')
            self.between_dt = getattr(args, 'between_dt', None)
            self.between_rng = random.Random(getattr(args, 'between_seed', 0))          # seeded once per trainer; host only
            self.between_flows = None            # test hook: the (T', 4, h, w) flows of the last between term
            self.between_frames = None           # test hook: its synthesized frames X (B, 2K, C, h, w)
            # at sampled points: N random (pair, tau, y, x) a step instead of whole grids; present only when given
            self.between_points = getattr(args, 'between_points', None)
            if self.between_points is not None:
                self.between_points = int(self.between_points)
                self.between_seed = int(getattr(args, 'between_seed', 0))
                self._between_gens = {}          # device -> torch.Generator, seeded once per trainer
                self.between_sample = None       # test hook: (pix, pair, tau, rev) of the last between term

        # the smoothness prior at sampled points: off unless the namespace carries a non-zero weight; the attributes exist only then
        self.smooth_at_weight = float(getattr(args, 'loss_smooth_at', 0) or 0)
        if self.smooth_at_weight != 0:
            self.loss_smooth_at = self.smooth_at_weight
            self.smooth_points = int(getattr(args, 'smooth_points', None) or 4096)
            self.smooth_seed = int(getattr(args, 'smooth_seed', 0))
            self._smooth_gens = {}               # device -> torch.Generator of its own: the --between-points draw is unchanged
            self.smooth_sample = None            # test hook: (pair, py, px, poses) of the last term

    # ---- the pieces of the step ----

    def _scale(self, scale, frame):
        """the flow scale of the batch as a Python float (flow_fields bakes it into the kernel's arguments): read from the batch
        once per frame size -- it is `W / 5` of the data set"""
        if not torch.is_tensor(scale):
            return float(scale)
        key = tuple(frame.shape[-2:])
        if key not in self._scales:
            self._scales[key] = float(scale.reshape(-1)[0])
        return self._scales[key]

    def forward(self, F, T, scale):
        """trainer.py:37-45: (flow12, flow21), each (t, 2, h, w), at the times T on the pixel grid of the frames F"""
        _, _, h, w = F.shape
        return flownet.flow_fields(self.net, T.to(torch.float32), h, w, self._scale(scale, F))

    def _epe(self, flow, gt):
        if self.fused:
            return flow_epe(flow, gt)
        return torch.sum((flow - gt) ** 2, dim=1).sqrt().mean().detach()

    def _splat_mask(self, mask, splat):
        if self.fused:
            return splat_mask(mask, splat)
        return mask * (splat != 0)

    def _no_occlusion(self, frame):
        """the reference's `torch.ones(2)` placeholders as an all-ones (n, 1, h, w) mask"""
        key = (frame.shape[0],) + tuple(frame.shape[-2:]) + (frame.device,)
        if key not in self._ones:
            self._ones[key] = torch.ones(frame.shape[0], 1, *frame.shape[-2:], device=frame.device)
        return self._ones[key]

    def log(self, name, value, on_step=True, on_epoch=False, batch_size=1, **_):
        """on_epoch without on_step (the EPEs): the mean over the epoch so far, weighted by batch size, kept on the device"""
        if on_epoch and not on_step and torch.is_tensor(value):
            total, count = self._epoch_means.get(name, (0.0, 0))
            total, count = total + value.detach() * batch_size, count + batch_size
            self._epoch_means[name] = (total, count)
            value = total / count
        super().log(name, value)

    def _new_epoch(self, prefix):
        for name in [k for k in self._epoch_means if k.startswith(prefix)]:
            del self._epoch_means[name]

    def losses(self, frame1, frame2, flow12, flow21):
        """trainer.py:50-74 after the network: the masks, the two splats and the four loss terms.  Returns
        (l1, census, ssim, smooth, (mask1, mask2, softmax1, softmax2))."""
        if self.occlusion:
            mask1 = self.occlusion(flow12, flow21, self.args.occl_thresh)
            mask2 = self.occlusion(flow21, flow12, self.args.occl_thresh)
        else:
            mask1 = mask2 = self._no_occlusion(frame1)
        _, metric = flow_warp_l1(frame1, flow21, frame2)
        softmax1 = FL.FunctionSoftsplat(frame2, flow21, -20 * metric, strType='softmax')
        mask1 = self._splat_mask(mask1, softmax1)
        _, metric = flow_warp_l1(frame2, flow12, frame1)
        softmax2 = FL.FunctionSoftsplat(frame1, flow12, -20 * metric, strType='softmax')
        mask2 = self._splat_mask(mask2, softmax2)

        l1_loss = self.l1(softmax1, frame1, mask1) + self.l1(softmax2, frame2, mask2)
        census_loss = self.census(softmax1, frame1, mask1) + self.census(softmax2, frame2, mask2)
        ssim_loss = self.ssim(softmax1, frame1, mask1) + self.ssim(softmax2, frame2, mask2)
        smooth_loss = self.smooth1(frame1, flow12) + self.smooth1(frame2, flow21)
        return l1_loss, census_loss, ssim_loss, smooth_loss, (mask1, mask2, softmax1, softmax2)

    def on_before_batch_transfer(self, batch, dataloader_idx=0):
        """Lightning's hook, called by the trainer while the batch is on the host: with the between loss on, keep the pairs' time
        stamps as Python floats, so that building the slot table reads nothing back from the device"""
        self._times_on_host = None
        if self.between_weight != 0 and torch.is_tensor(batch[2]) and not batch[2].is_cuda:
            self._times_on_host = [float(t) for t in batch[2].reshape(-1).tolist()]
        return batch

    def _host_times(self, times):
        """the batch's stamps as Python floats: what `on_before_batch_transfer` kept; a caller that hands `training_step` a device
        batch directly pays one read of B floats"""
        kept, self._times_on_host = getattr(self, '_times_on_host', None), None
        if kept is not None and len(kept) == times.numel():
            return kept
        return [float(t) for t in times.detach().reshape(-1).cpu().tolist()]

    def between_table(self, times, taus):
        """(stamps, slots, blend) of the between term: `gather_slots(times, taus, dt, back)`, its table repeated along K to
        (B, 2K, 6), and the blend weights [0] * K + [1] * K: rows 0 .. K-1 read frame 1 alone (A), rows K .. 2K-1 frame 2 alone (B)"""
        from . import flowsynth
        stamps, slots = flowsynth.gather_slots(times, taus, self.between_dt, self.between_back)
        k = len(taus)
        return stamps, torch.cat([slots, slots], dim=1).contiguous(), [0.0] * k + [1.0] * k

    def between_loss(self, frame1, frame2, times, scale):
        """weight * mean |A - B| at K fresh times tau ~ U(0, 1) drawn on the host: A = (W0 + e I0(p)) / (n0 + e) and
        B = (W1 + e I1(p)) / (n1 + e) are two rows of one `gather` call whose flows come from one more `flow_fields` call, with
        gradient, at the in-between stamps.  `times` is the host list of the batch's stamps."""
        from . import flowsynth
        k = self.between_taus
        taus = [self.between_rng.random() for _ in range(k)]
        taus = [t if t > 0.0 else 0.5 for t in taus]                 # random() is in [0, 1): keep tau inside (0, 1)
        stamps, table, blend = self.between_table(times, taus)
        at = torch.tensor(stamps, dtype=torch.float32, device=frame1.device)
        per = max(1, GRID_POINTS // (frame1.shape[-2] * frame1.shape[-1]))
        parts = [torch.cat(self.forward(frame1, at[i:i + per], scale), dim=1) for i in range(0, len(stamps), per)]
        flows = parts[0] if len(parts) == 1 else torch.cat(parts)
        synth = flowsynth.gather if self.fused else flowsynth.gather_composed
        frames = synth(frame1, frame2, flows, table, blend, flow_grad=True)
        self.between_flows, self.between_frames = flows, frames
        return self.between_weight * (frames[:, :k] - frames[:, k:]).abs().mean()

    def between_points_table(self, times, b, h, w):
        """The point list of one step, drawn with torch ops on the device of `times` from a generator seeded once per
        trainer; nothing is read back.  pair ~ U{0 .. B-1}, tau ~ U[0, 1), py ~ U[0, H-1], px ~ U[0, W-1]; the poses
        (times[pair] + tau dt, 2 py / (H-1) - 1, 2 px / (W-1) - 1), and under back='network' the same poses at s - dt, with rev set
        where s - dt lies before the clip's first stamp (-1; `gather_slots`' slack of dt / 1000).  Returns
        (pix (N, 2), pair (N,) int32, tau (N,), rev (N,) bool or None, [poses (N, 3) per slab])."""
        dev, n, dt = times.device, self.between_points, float(self.between_dt)
        if dev not in self._between_gens:
            self._between_gens[dev] = torch.Generator(device=dev).manual_seed(self.between_seed)
        gen = self._between_gens[dev]
        pair = torch.randint(0, b, (n,), generator=gen, device=dev, dtype=torch.int32)
        u = torch.rand(3, n, generator=gen, device=dev, dtype=torch.float32)
        tau, py, px = u[0], u[1] * (h - 1), u[2] * (w - 1)
        s = times.detach().to(torch.float32).reshape(-1)[pair.long()] + tau * dt
        ys, xs = 2 * py / max(h - 1, 1) - 1, 2 * px / max(w - 1, 1) - 1
        poses, rev = [torch.stack((s, ys, xs), dim=1)], None
        if self.between_back == 'network':
            before = s - dt
            rev = before < -1.0 - 1e-3 * dt
            poses.append(torch.stack((before, ys, xs), dim=1))
        return torch.stack((py, px), dim=1), pair, tau, rev, poses

    def between_points_loss(self, frame1, frame2, times, scale):
        """weight * mean |A - B| at N fresh points: the network at the N (under back='network' 2 N) poses through `flow_at`, one call
        a slab, then one `gather_at` call with blends 0 and 1 and its gradient to the flows.  `times`: the batch's stamps, on the
        device."""
        from . import flowsynth
        b, _, h, w = frame1.shape
        pix, pair, tau, rev, poses = self.between_points_table(times, b, h, w)
        factor = self._scale(scale, frame1)
        flows = torch.stack([flownet.flow_at(self.net, p, factor, planar=True) for p in poses])
        synth = flowsynth.gather_at if self.fused else flowsynth.gather_at_composed
        out = synth(frame1, frame2, flows, pix, pair, tau, rev, blend=(0.0, 1.0), flow_grad=True)
        self.between_flows, self.between_frames, self.between_sample = flows, out, (pix, pair, tau, rev)
        return self.between_weight * (out[0] - out[1]).abs().mean()

    def smooth_points_table(self, times, b, h, w):
        """(pair (N,) int64, py (N,), px (N,), poses (N, 3)) of one step: pair ~ U{0 .. B-1}, py ~ U[0, H-1], px ~ U[0, W-1] from a device
        generator seeded once per trainer (`smooth_seed`); nothing is read back"""
        dev, n = times.device, self.smooth_points
        if dev not in self._smooth_gens:
            self._smooth_gens[dev] = torch.Generator(device=dev).manual_seed(self.smooth_seed)
        gen = self._smooth_gens[dev]
        pair = torch.randint(0, b, (n,), generator=gen, device=dev)
        u = torch.rand(2, n, generator=gen, device=dev, dtype=torch.float32)
        py, px = u[0] * (h - 1), u[1] * (w - 1)
        t = times.detach().to(torch.float32).reshape(-1)[pair]
        poses = torch.stack((t, 2 * py / max(h - 1, 1) - 1, 2 * px / max(w - 1, 1) - 1), dim=1)
        return pair, py, px, poses

    @staticmethod
    def _sample_clamped(img, pair, py, px):
        """img (B, C, H, W) at (pair, py, px): bilinear with clamped taps, torch index arithmetic; (N, C)"""
        h, w = img.shape[-2:]
        y0, x0 = py.floor(), px.floor()
        fy, fx = (py - y0)[:, None], (px - x0)[:, None]
        y0i, x0i = y0.long().clamp(0, h - 1), x0.long().clamp(0, w - 1)
        y1i, x1i = (y0.long() + 1).clamp(0, h - 1), (x0.long() + 1).clamp(0, w - 1)
        top = img[pair, :, y0i, x0i] * (1 - fx) + img[pair, :, y0i, x1i] * fx
        bottom = img[pair, :, y1i, x0i] * (1 - fx) + img[pair, :, y1i, x1i] * fx
        return top * (1 - fy) + bottom * fy

    def smooth_at_loss(self, frame1, frame2, times, scale):
        """W * sum over (channels 0:2 guided by frame1, 2:4 by frame2) of 0.5 (mean(w_y robust_l1(gy)) + mean(w_x robust_l1(gx))): the
        reference's BilateralSmooth of order 1 with its finite difference over the pixel grid replaced by the network's analytic derivative
        at N random points, gy / gx the flow change per pixel (image_grads' unit).  One flow_at(.., jacobian='yx') call (fused = False:
        flow_jacobian_composed)"""
        b, _, h, w = frame1.shape
        pair, py, px, poses = self.smooth_points_table(times, b, h, w)
        factor = self._scale(scale, frame1)
        if self.fused:
            _, jac = flownet.flow_at(self.net, poses, factor, planar=True, jacobian='yx')
        else:
            _, jac = flownet.flow_jacobian_composed(self.net, poses, factor, 'yx', planar=True)
        self.smooth_sample = (pair, py, px, poses)
        gy, gx = jac[0] * (2.0 / max(h - 1, 1)), jac[1] * (2.0 / max(w - 1, 1))          # (4, N) each
        gauss, k = self.args.edge_func == 'gauss', float(self.args.edge_constant)

        def edge(d):
            d = k * d
            return torch.exp(-(d * d if gauss else d.abs()).mean(dim=1))

        def robust(v):
            return torch.sqrt(v * v + 1e-6)

        total = 0
        for ch, img in ((slice(0, 2), frame1), (slice(2, 4), frame2)):
            img = img.detach().to(torch.float32)
            at = self._sample_clamped(img, pair, py, px)
            w_y = edge(self._sample_clamped(img, pair, py + 1, px) - at)
            w_x = edge(self._sample_clamped(img, pair, py, px + 1) - at)
            total = total + 0.5 * ((w_y[None] * robust(gy[ch])).mean() + (w_x[None] * robust(gx[ch])).mean())
        return self.smooth_at_weight * total

    # ---- the LightningModule surface ----

    def training_step(self, batch, batch_idx):
        """trainer.py:47-87.  `batch`: (frame1, frame2, times, scale) and, with ground truth, the flow from frame1 to frame2."""
        frame1, frame2, times, scale = batch[:4]
        if batch_idx == 0:
            self._new_epoch('train/')
        if self.between_weight != 0:
            # before the step's own flow_fields call: a spatial controller stashes at the grid evaluated LAST, the frame times'
            if self.between_points is not None:
                between_loss = self.between_points_loss(frame1, frame2, times, scale)
            else:
                between_loss = self.between_loss(frame1, frame2, self._host_times(times), scale)
        if self.smooth_at_weight != 0:
            smooth_at_loss = self.smooth_at_loss(frame1, frame2, times, scale)
        flow12, flow21 = self.forward(frame1, times, scale)
        if len(batch) == 5:
            self.log('train/EPE', self._epe(flow12, batch[-1]), on_step=False, on_epoch=True, batch_size=frame1.shape[0])
        flow12, flow21 = flow12.contiguous(), flow21.contiguous()
        l1_loss, census_loss, ssim_loss, smooth_loss, (mask1, mask2, softmax1, softmax2) = self.losses(frame1, frame2, flow12, flow21)
        loss = l1_loss + census_loss + ssim_loss + smooth_loss
        if self.between_weight != 0:
            loss = loss + between_loss
        if self.smooth_at_weight != 0:
            loss = loss + smooth_at_loss
        if hasattr(self.net, 'stash_grid'):
            # a spatial controller updates its mask grid in place and the backward pass checks the grid's version: on_after_backward stashes
            self._stash = tuple(t.detach() for t in (softmax1, frame1, mask1, softmax2, frame2, mask2))
        else:
            self.net.stash_iteration(loss.detach())

        self.log('train/loss', loss)
        self.log('train/loss_epoch', loss, on_step=False, on_epoch=True, batch_size=frame1.shape[0])
        self.log('train/l1', l1_loss)
        self.log('train/census', census_loss)
        if self.ssim.weight != 0:
            self.log('train/ssim', ssim_loss)
        self.log('train/smooth', smooth_loss)
        if self.between_weight != 0:
            self.log('train/between', between_loss)
        if self.smooth_at_weight != 0:
            self.log('train/smooth_at', smooth_at_loss)
        return loss

    def on_after_backward(self):
        """Lightning's hook, called by the trainer between backward() and the optimizer's step.  Under a StashedSpatialController: the
        per-point loss of this step goes into the controller's log (`stash_grid`: the fused `error_stash`, or with `fused = False`
        the composed form), and after `block_iterations` of them `update_progress()` closes the fitted cells, opens the next block in the
        others and resets `iteration` -- the `(step + 1) % block_iterations == 0` of tools/fit_flow.py."""
        stash, self._stash = self._stash, None
        if stash is None:
            return
        self.net.stash_grid(*stash, fused=self.fused)
        if self.net.iteration >= self.net.block_iterations:
            self.net.update_progress()

    def on_train_end(self):
        self.completed_training = True

    def validation_step(self, batch, batch_idx):
        """trainer.py:93-98.  Under `flowdata.Holdout` (a batch of six: the pair, the held-out frames and their times) there is no
        ground-truth flow: `val/PSNR` and `val/SSIM`, the means over the held-out frames, are logged in place of `val/EPE`."""
        frame1, _, times, scale = batch[:4]
        if batch_idx == 0:
            self._new_epoch('val/')
        if len(batch) == 6:
            held, taus = batch[4], batch[5][0]
            net = self.holdout_quality(batch, held, taus)['net']
            count = held.shape[0] * held.shape[1]
            self.log('val/PSNR', net.psnr.mean(), on_step=False, on_epoch=True, batch_size=count)
            self.log('val/SSIM', net.ssim.mean(), on_step=False, on_epoch=True, batch_size=count)
            return
        flow_fw, _ = self.forward(frame1, times, scale)
        self.log('val/EPE', self._epe(flow_fw, batch[4]), on_step=False, on_epoch=True, batch_size=frame1.shape[0])

    def test_step(self, batch, batch_idx):
        """trainer.py:100-112: the colour-coded forward flow (uint8, on the device), the occlusion mask as 0 / 255 bytes (host)
        and, with ground truth, the batch's EPE"""
        frame1, _, times, scale = batch[:4]
        flow_fw, flow_bw = self.forward(frame1, times, scale)
        out = {'flow': flow2img(flow_fw)}
        if self.occlusion:
            out['mask'] = (self.occlusion(flow_fw, flow_bw, self.args.occl_thresh).type(torch.uint8) * 255).cpu()
        if len(batch) == 5:
            out['epe'] = self._epe(flow_fw, batch[-1])
        return out

    def test_epoch_end(self, outputs):
        """trainer.py:114-132: results/flow_<tag>_epe_<epe:.3f>.gif (and results/occl_<tag>.gif); returns the mean EPE"""
        epe = torch.stack([seq['epe'] for seq in outputs]).mean().item() if 'epe' in outputs[0] else 0
        flows = torch.cat([seq['flow'] for seq in outputs], dim=0)
        os.makedirs('results', exist_ok=True)
        save_gif(f'results/flow_{self.test_tag}_epe_{epe:.3f}.gif', flows.permute(0, 2, 3, 1).cpu().numpy())
        if self.occlusion:
            masks = torch.cat([seq['mask'] for seq in outputs], dim=0)
            save_gif(f'results/occl_{self.test_tag}.gif', masks.permute(0, 2, 3, 1).numpy())
        print(f'test/EPE {epe:.6f}')
        if self.logger:
            self.logger.log_metrics({'test/EPE': epe, 'epoch': self.current_epoch}, getattr(self.trainer, 'global_step', 0))
        return epe

    def visibility_masks(self, flow12, flow21, occlusion):
        """(mask1, mask2) of the step (`losses`) before the splat masks, from the flows at the frame times: `occlusion` is 'wang' or
        'brox', the operators of `flowloss`, with the trainer's `occl_thresh`"""
        op = {'wang': FL.occlusion_wang, 'brox': FL.occlusion_brox}[occlusion]
        return op(flow12, flow21, self.args.occl_thresh), op(flow21, flow12, self.args.occl_thresh)

    def interpolate(self, batch, taus, synthesis='splat', dt=None, back='network', occlusion=None, **kw):
        """The frames at `taus` in [0, 1] between frame1 and frame2 of `batch` (frame1, frame2, times, scale, ...), (n, K, 3, h, w):
        the network's two flows at the batch's time stamps, then `flowsynth.synthesize` (its keywords pass through).  No gradient;
        the network is evaluated in eval() and left in the mode it was found in.

        synthesis='gather' (DESIGN 19): the network is asked for its flows at the in-between times themselves -- one `flow_fields`
        call at the stamps of `flowsynth.gather_slots(times, taus, dt, back)`; several, joined, where the stamps times h w exceed
        the 2^22 points one call takes -- and `flowsynth.gather` reads both frames through them (its keywords pass through).  `dt`: the spacing of the clip's times, 2 / (frames - 1); back='reverse' evaluates half the stamps
        and uses the negated forward flow for the previous frame.

        occlusion='wang' | 'brox' (synthesis='gather' only): the occlusion-aware rule.  The network's two flows at the
        batch's time stamps -- what the splat path evaluates -- give the step's mask1 and mask2 (`visibility_masks`), and `gather`
        takes them as `visible=(mask1, mask2)`."""
        from . import flowsynth
        frame1, frame2, times, scale = batch[:4]
        if synthesis not in ('splat', 'gather'):
            raise ValueError(f"interpolate: synthesis is 'splat' or 'gather', got {synthesis!r}")
        if occlusion not in (None, 'wang', 'brox'):
            raise ValueError(f"interpolate: occlusion is None, 'wang' or 'brox', got {occlusion!r}")
        if occlusion is not None and synthesis != 'gather':
            raise ValueError("interpolate: occlusion= is the masked gather rule and needs synthesis='gather'")
        if synthesis == 'gather':
            if dt is None:
                raise ValueError("interpolate: synthesis='gather' evaluates the network between the frames and needs dt, the spacing "
                                 'of the clip\'s times (2 / (frames - 1))')
            dim = int(self.net.domain_dim)
            if dim != 3:
                raise ValueError(f"domain_dim {dim}: synthesis='gather' asks the network for a time between two frames; a network on "
                                 '(y, x) has no time axis')
            stamps, slots = flowsynth.gather_slots(times, taus, dt, back)
        was_training = self.net.training
        self.net.eval()
        try:
            with torch.no_grad():
                if synthesis == 'gather':
                    at = torch.tensor(stamps, dtype=torch.float32, device=frame1.device)
                    # one flow_fields call where its grid limit allows (T h w <= 2^22 points), else as few as fit, joined by one copy
                    per = max(1, GRID_POINTS // (frame1.shape[-2] * frame1.shape[-1]))
                    parts = [flowsynth.joined_flows(*self.forward(frame1, at[i:i + per], scale)) for i in range(0, len(stamps), per)]
                    flows = parts[0] if len(parts) == 1 else torch.cat(parts)
                    if occlusion is not None:
                        kw = dict(kw, visible=self.visibility_masks(*self.forward(frame1, times, scale), occlusion))
                    return flowsynth.gather(frame1, frame2, flows, slots, taus, **kw)
                flow12, flow21 = self.forward(frame1, times, scale)
                return flowsynth.synthesize(frame1, frame2, flow12, flow21, taus, **kw)
        finally:
            self.net.train(was_training)

    def holdout_quality(self, batch, held, taus, quantize=True, frames=None, synthesis='splat', dt=None, back='network',
                        occlusion=None):
        """Score the frames synthesized at `taus` between the pair of `batch` against the real frames `held` (n, K, 3, h, w): a dict of
        `flowsynth.Quality`, each entry (n, K) -- 'net': `interpolate(batch, taus)`; and, through the same operator, the two
        baselines that use no flow, 'blend': (1 - tau) frame1 + tau frame2, and 'repeat': the nearer source frame (frame1 up to
        tau = 0.5).  `quantize=True` measures all three as bytes, as the written PNGs hold them.  `frames`: what `interpolate(batch, taus)`
        returned, for a caller that has it already (the splat adds with atomics: a second call may differ in the last bits).
        `synthesis`, `dt`, `back`, `occlusion`: how 'net' is synthesized where `frames` is None, as `interpolate` takes them."""
        from . import flowsynth
        frame1, frame2 = batch[0], batch[1]
        values = flowsynth._host_taus(taus)
        with torch.no_grad():
            net = self.interpolate(batch, values, synthesis=synthesis, dt=dt, back=back, occlusion=occlusion) if frames is None else frames
            tau = torch.tensor(values, dtype=frame1.dtype, device=frame1.device).view(1, -1, 1, 1, 1)
            blend = (1 - tau) * frame1[:, None] + tau * frame2[:, None]
            repeat = torch.where(tau <= 0.5, frame1[:, None], frame2[:, None])
            held = held.to(frame1.device)
            return {name: flowsynth.quality(frames, held, quantize=quantize)
                    for name, frames in (('net', net), ('blend', blend), ('repeat', repeat))}

    def configure_optimizers(self):
        return FusedLAMB(self.net.parameters(), lr=self.lr)

    # ---- checkpoints ----

    def load_state_dict(self, state_dict, strict=True):
        """nn.Module's loader fills `net.mask_stashed` without calling the controller's own load_state_dict: rebuild the mask here"""
        out = super().load_state_dict(state_dict, strict)
        if hasattr(self.net, 'load_mask'):
            with torch.no_grad():
                self.net.load_mask()
        return out

    def on_load_checkpoint(self, checkpoint):
        """Resume the controller's schedule: one `stash_iteration` per step, so `iteration` is the checkpoint's global step; the
        blocks opened so far are the whole blocks inside floor(mask_stashed), but never ahead of the schedule (a fully ramped
        block counts as open in the sum half a period before the controller moves on).

        A StashedSpatialController keeps one mask per cell, so `mask_stashed` has res^3 entries and no single one speaks for the schedule:
        `cur_block` is the largest multiple of `block_size` not above floor(max(mask_stashed)) (the cell that got furthest; never below
        `block_size`), `next_block` follows from it by the class's rule, and `iteration = global_step % block_iterations`
        (`update_progress` resets it every `block_iterations` steps).  `in_progress`, `log_buffer` and `log_counter` are registered
        buffers: the state dict has restored them already."""
        net = self.net
        if not hasattr(net, 'cur_block'):
            return
        if hasattr(net, 'stash_grid'):
            bs, dim = net.block_size, net.encoding_dim
            opened = int(torch.floor(net.mask_stashed.max()))
            net.cur_block = max(opened // bs * bs, bs)
            net.next_block = net.cur_block + bs
            if dim - net.next_block < bs:
                net.next_block = dim
            net.iteration = int(checkpoint.get('global_step', 0)) % max(net.block_iterations, 1)
            print(f'resumed: iteration {net.iteration}, controller cur_block {net.cur_block} / {dim}')
            return
        net.iteration = int(checkpoint.get('global_step', 0))
        bs, dim = net.block_size, net.encoding_dim
        opened = int(torch.floor(net.mask_stashed.reshape(-1)[0]))
        scheduled = bs * (1 + min(net.iteration, net.progress_iterations) // max(net.block_iterations, 1))
        cur = dim if opened >= dim else max(bs, min(opened // bs * bs, scheduled))
        nxt = min(cur + bs, dim)
        if dim - nxt < bs:
            nxt = dim
        net.cur_block, net.next_block = cur, nxt
        print(f'resumed: iteration {net.iteration}, controller cur_block {net.cur_block} / {dim}')

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, args, test_tag=None, map_location=None):
        """pl.LightningModule.load_from_checkpoint as main.py:88, 117 uses it"""
        model = cls(args, test_tag=test_tag)
        ck = load_checkpoint(checkpoint_path, map_location=map_location or 'cpu')
        model.load_state_dict(ck['state_dict'])
        model.on_load_checkpoint(ck)
        return model
