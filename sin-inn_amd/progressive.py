"""The controllers of the progressive encoding (video-interpolation/progressive_controller.py:14-158): a module around a
progressive model (`sin_inn_amd.flownet.PRBFModel` / `PFFModel` / `PUFFModel` / .. / `MPFFModel`) that owns the per-feature mask and opens it
block by block as training goes on, as video-interpolation/main.py:136-143 wraps every `is_progressive` network.

    ProgressiveEncoderController   progressive_controller.py:14-92
    LinearController               progressive_controller.py:95-132
    LinearControllerEarly          progressive_controller.py:135-158   (the one main.py uses unless --spatially-adaptive is given)
    StashedSpatialController       progressive_controller.py:461-710   (what --spatially-adaptive builds)

The mask is HOST state (a CPU tensor of `encoding_dim` = 515 values), as in the reference, and so is everything that decides it.
`device_mask(device)` hands the kernels a device copy and `k_active`, the number of leading features after which the mask is all
zero; the copy is refreshed by a pinned, non-blocking upload only when the host mask differs from what was uploaded last.  A
refresh makes a new device tensor, so a backward pass that still holds the mask of its forward pass keeps the right one.

The port keeps the reference's state-dict keys (`mask_stashed`, `model.encode.*`, `model.model.model.N.*`) and its quirks, which
checkpoints and training curves depend on:
  * `not self.train()` in update_mask is always false and puts the module in training mode;
  * LinearControllerEarly.stash_iteration calls `super(LinearController, self)`: it skips LinearController in the MRO;
  * a checkpoint keeps `mask_stashed`, the SUM of the mask, and load_mask rebuilds `floor(sum)` ones followed by the fraction:
    a block of six entries ramping at 0.5 comes back as three ones.
Calling a linear controller on a pose list, `controller(poses, override_mask=, get_mask=)`, is progressive_controller.py:45-53 on
`flownet.flow_at`; `flow_fields` evaluates a controller on a grid.  StashedSpatialController does both: `controller(poses)` is its
reference form (progressive_controller.py:670-680), the interpolation inside the kernels; `mask_by` / `expand_by` stay out.

StashedSpatialController keeps a mask PER GRID CELL, [res^3][515], and every point reads the trilinear interpolation of its box
blur.  At res = 50 that is 257 MB, so unlike the linear controllers its state lives on the DEVICE, next to the model (`.to()` /
`.cuda()` move it), nothing is uploaded per step, and the blurred grid the kernels sample is cached and updated IN PLACE: between
two `increase_block` calls only the six columns of the block in progress change and only they are blurred again.  A backward pass
must therefore run before the next `stash_iteration` / `stash_grid` / `update_progress` (flow_fields checks the grid's version and raises
otherwise).  The box blurs (mask and loss log) are sums of shifted slices, axis by axis, in a fixed order instead of the reference's
conv3d: the same numbers to fp32 rounding, bitwise the same whether six columns or all 515 are blurred, and no convolution library
in a training step.  `stash_iteration` takes the per-point loss the class is written for; the reference's own trainer passes a
scalar there and fails with an IndexError, here that is a ValueError that says so.  `stash_grid` is the form the flow trainer uses
(`main.py --spatially-adaptive`): it takes the six tensors of the step's two L1 terms, and one fused operator computes the per-point
loss on the grid evaluated last and SUMS it into the log, cell by cell in a fixed order (csrc/flowtrain.hip).

Every 515-wide progressive network runs under every controller here, `MPFFModel` (the piecewise-linear encoding) included; `PPEModel`
(27 wide) under the linear ones only.

Out of scope: FixedSpatialController, AdaptiveController, `mask_dim` other than the three coordinates, and a fused stash for pose
lists (they stay on `stash_iteration`).
"""
import torch
import torch.nn as nn

from .flownet import Mask, flow_at, last_open


class ProgressiveEncoderController(nn.Module):
    """progressive_controller.py:14-92."""

    @property
    def is_progressive(self):
        return True

    def update_progress(self):
        return

    @property
    def name(self):
        raise NotImplementedError

    def stash_iteration(self, *args):
        self.iteration += 1
        with torch.no_grad():
            self.update_mask()

    @property
    def encoding_dim(self):
        return self.model.encoding_dim

    @property
    def domain_dim(self):
        return self.model.domain_dim

    def update_mask(self):
        raise NotImplementedError

    def __call__(self, x, **kwargs):
        """progressive_controller.py:45-53 on flow_at: the controller's own mask goes through `device_mask` (uploaded when it changed,
        with its k_active), an `override_mask` as flow_at takes it; `get_mask` among the keywords returns (out, that mask); `pose_grad=True` is flow_at's"""
        override_mask = kwargs.get('override_mask')
        if override_mask is not None and override_mask.dim() == 2:    # a grid (res^3, 515): the per-point mask, interpolated by the kernels
            return flow_at(self, x, 1.0, override_mask=override_mask, get_mask='get_mask' in kwargs, pose_grad=kwargs.get('pose_grad', False),
                           jacobian=kwargs.get('jacobian'))
        out = flow_at(self, x, 1.0, override_mask=override_mask, pose_grad=kwargs.get('pose_grad', False), jacobian=kwargs.get('jacobian'))
        if 'get_mask' in kwargs:
            return out, self.mask if override_mask is None else override_mask
        return out

    def init_mask(self):
        return torch.ones(self.model.encoding_dim)

    def load_mask(self):
        mask = torch.zeros(self.mask_stashed.shape[0], self.encoding_dim)
        arange = torch.arange(self.encoding_dim)
        arange = arange.unsqueeze(0).repeat(self.mask_stashed.shape[0], 1)
        fill_a = arange.lt(torch.floor(self.mask_stashed[:, None]).cpu())
        fill_b = ~fill_a * arange.le(self.mask_stashed[:, None].cpu())
        mask[fill_a] = 1
        mask[fill_b] = (self.mask_stashed[self.mask_stashed.lt(self.encoding_dim)] % 1).cpu()
        self.mask = mask.detach()

    def load_state_dict(self, state_dict, strict=True):
        super().load_state_dict(state_dict, strict)
        with torch.no_grad():
            self.load_mask()
            # the reference moves the mask next to `mask_stashed`; here the mask stays on the host (device_mask uploads it)

    def save_mask(self):
        self.mask_stashed = self.mask.sum(-1).to(self.mask_stashed.device)
        if len(self.mask_stashed.shape) == 0:
            self.mask_stashed = self.mask_stashed.unsqueeze(0)

    def state_dict(self, *args, **kwargs):
        self.save_mask()
        return super().state_dict(*args, **kwargs)

    def linears(self):
        return self.model.linears()

    def device_mask(self, device):
        """Mask(mask on `device`, k_active); uploads only if the host mask changed since the last call for this device"""
        device = torch.device(device)
        hit = self._device_masks.get(device)
        if hit is None or not torch.equal(hit[0], self.mask):
            host = self.mask.detach().to(torch.float32).contiguous()
            assert host.dim() == 1 and host.numel() == self.encoding_dim, 'a global mask of encoding_dim values'
            snapshot = host.clone()
            hit = (snapshot, snapshot.pin_memory().to(device, non_blocking=True), last_open(snapshot))
            self._device_masks[device] = hit
            self.uploads += 1
        return Mask(hit[1], hit[2])

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.mask = self.init_mask().detach()
        if self.mask.dim() > 1:
            mask_stashed = torch.zeros(self.mask.shape[0])
        else:
            mask_stashed = torch.zeros(1)
        self.register_buffer('mask_stashed', mask_stashed.detach())
        self.iteration = 0
        self._device_masks = {}
        self.uploads = 0


class LinearController(ProgressiveEncoderController):
    """progressive_controller.py:95-132."""

    def load_mask(self):
        super().load_mask()
        self.mask = self.mask.squeeze_()

    @property
    def name(self):
        return 'linear'

    def increase_block(self):
        self.mask[self.cur_block:  self.next_block] = 1
        self.cur_block = self.next_block
        self.next_block += self.block_size
        if self.model.encoding_dim - self.next_block < self.block_size:
            self.next_block = self.model.encoding_dim

    def update_mask(self):
        if not self.train() or self.iteration > self.progress_iterations:
            return
        elif self.iteration % self.block_iterations == 0:
            self.increase_block()
        else:
            alpha = min(1., float(2 * (self.iteration % self.block_iterations)) / self.block_iterations)
            self.mask[self.cur_block:  self.next_block] = alpha

    def __init__(self, model, max_iteration=1000, num_blocks=None):
        super().__init__(model)
        if num_blocks is None:
            self.block_size = model.domain_dim * 2
            num_blocks = (self.encoding_dim - self.block_size) // self.block_size
        else:
            self.block_size = self.encoding_dim // num_blocks
        self.mask[self.block_size:] = 0
        self.cur_block = self.block_size
        self.next_block = self.block_size * 2
        self.block_iterations = 3 * max_iteration // (4 * num_blocks)
        self.progress_iterations = self.block_iterations * num_blocks


class LinearControllerEarly(LinearController):
    """progressive_controller.py:135-158."""

    @property
    def name(self):
        return 'linear_early'

    def stash_iteration(self, loss):
        self.best_score = min(self.best_score, loss.mean().item())
        if self.best_score < self.epsilon and not self.trigger:
            print(f"progress stopped: {self.cur_block} / {self.encoding_dim}")
            self.trigger = True
        super(LinearController, self).stash_iteration(loss)

    def update_mask(self):
        if self.best_score < self.epsilon:
            return
        return super().update_mask()

    def __init__(self, model, max_iteration=1000, epsilon=1e-5, num_blocks=None):
        super().__init__(model, max_iteration, num_blocks)
        self.trigger = False
        self.epsilon = epsilon
        self.best_score = 10000


def _box_sum(x, k):
    """sum over the k^3 box around every cell of x (res, res, res, C), replicate padding: axis by axis, k shifted slices added in
    index order.  Elementwise in C: a subset of columns gives bitwise the columns of the whole"""
    mk, res = k // 2, x.shape[0]
    idx = torch.arange(-mk, res + mk, device=x.device).clamp_(0, res - 1)
    for dim in range(3):
        padded = x.index_select(dim, idx)
        x = padded.narrow(dim, 0, res).clone()
        for j in range(1, k):
            x += padded.narrow(dim, j, res)
    return x


class StashedSpatialController(ProgressiveEncoderController):
    """progressive_controller.py:461-710, `mask_dim == domain_dim == 3`.  State on the device of the model (see the module text)."""

    @property
    def epsilon(self):
        if type(self.epsilon_) is float:
            return self.epsilon_
        elif self.iteration >= self.progress_iterations:
            return self.epsilon_[-1]
        else:
            return self.epsilon_[0] + (float(self.iteration) / self.progress_iterations) * (self.epsilon_[1] - self.epsilon_[0])

    @property
    def name(self):
        return 'stash_spatial'

    # ---- where the state lives ----
    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.mask = fn(self.mask)
        self.mask_ = None
        self.stash = (None, None)
        return out

    def centre_scale_host(self):
        """centre (t, y, x), scale (t, y, x): the six host floats the kernels take"""
        return tuple(float(v) for v in self.center_scale.reshape(-1))

    def scale_dummy(self, x):
        return x

    def scale_real(self, x):
        cs = self.center_scale.to(x.device)
        return (x - cs[0]) * cs[1]

    def set_scale(self, training_points):
        """the second of the reference's two definitions, which is the one in force (they are the same)"""
        max_vals, min_vals = training_points.max(0)[0], training_points.min(0)[0]
        self.center_scale[0, 0] = ((max_vals + min_vals) / 2).to(self.center_scale.device)
        self.center_scale[1, 0] = (2 / (max_vals - min_vals)).to(self.center_scale.device)
        self.scale = self.scale_real

    # ---- the loss log ----
    def stash_iteration(self, loss, *args):
        if loss.dim() == 0:
            raise ValueError('StashedSpatialController.stash_iteration needs a per-point loss of shape (N,), one value per point of '
                             'the last evaluated grid; got a 0-d tensor')
        loss = loss.clone().detach()
        with torch.no_grad():
            inds, alphas = self.stash
            if inds is None:
                inds, alphas = self.stash = self.cells(self._last_poses())
            loss = (loss[:, None] * alphas).flatten()
            inds = inds.flatten()
            self.log_buffer[inds] += loss                # the reference's indexed +=: where indices repeat, one write stays
            self.log_counter[inds] += alphas.flatten()
        super().stash_iteration(loss)

    def stash_grid(self, softmax1, frame1, mask1, softmax2, frame2, mask2, fused=True):
        """The unsupervised step's form of stash_iteration: the per-point loss E of `flowtrainer.error_stash` at the points of the grid
        `flow_fields` evaluated last, added to the log as a SUM over the points of a cell, in a fixed order (stash_iteration keeps the
        reference's indexed `+=`: one write per repeated index); then `iteration += 1` and `update_mask()` as every stash does.
        `fused=False`: the composed form (`cells` of the flat point list and index_add_).  Call it after the backward pass: update_mask
        changes the mask grid in place."""
        from . import flowtrainer
        if self._last_grid is None:
            raise RuntimeError('stash_grid: the last evaluation was a pose list; its stash is stash_iteration(loss per point)'
                               if self._last_list is not None else 'stash_grid before any evaluation: no points to attribute the loss to')
        times, ys, xs = self._last_grid
        if (times.numel(), ys.numel(), xs.numel()) != (frame1.shape[0], frame1.shape[-2], frame1.shape[-1]):
            raise ValueError(f'stash_grid: the grid evaluated last has {times.numel()} x {ys.numel()} x {xs.numel()} points, the frames '
                             f'are {tuple(frame1.shape)}')
        with torch.no_grad():
            if fused:
                flowtrainer.error_stash(softmax1, frame1, mask1, softmax2, frame2, mask2, times, ys, xs, self.res,
                                        self.centre_scale_host(), self.log_buffer, self.log_counter)
            else:
                flowtrainer.error_stash_composed(softmax1, frame1, mask1, softmax2, frame2, mask2, times, ys, xs, self.cells,
                                                 self.log_buffer, self.log_counter)
        ProgressiveEncoderController.stash_iteration(self)

    def reset_buffer_(self):
        self.log_buffer[:] = 0
        self.log_counter[:] = 0
        self.iteration = 0

    def convolove_log(self, log_buffer, empty_log):
        """convolove_log_: cells nobody visited take the mean of their neighbours, then the box blur"""
        k3 = self.k ** 3
        log_buffer = log_buffer.view(self.res, self.res, self.res, 1)
        if self._any(empty_log):
            empty = empty_log.view(self.res, self.res, self.res, 1)
            around = (_box_sum(log_buffer, self.k) - log_buffer) * (1.0 / (k3 - 1))
            log_buffer = torch.where(empty, around, log_buffer)
        return (_box_sum(log_buffer, self.k) * (1.0 / k3)).flatten()

    @staticmethod
    def _any(t):
        return bool(t.any())

    @property
    def not_visited_mask(self):
        return self.log_counter.eq(0)

    @property
    def visited_percent(self):
        not_visited = float(self.not_visited_mask.sum().item())
        return 1 - not_visited / float(self.log_counter.numel())

    def update_progress(self):
        with torch.no_grad():
            empty_log = self.not_visited_mask
            self.log_counter[empty_log] = 1
            log_buffer = self.log_buffer / self.log_counter
            log_buffer = self.convolove_log(log_buffer, empty_log)
            self.in_progress = self.in_progress * log_buffer.gt(self.epsilon)
            self._in_progress_any = self._any(self.in_progress)
            self.increase_block()
            self.reset_buffer_()

    def is_full(self):
        num_non_zero = self.log_counter.nonzero().shape[0]
        return num_non_zero == self.mask.shape[0]

    # ---- the mask ----
    def _set_block(self, value):
        cols = self.mask[:, self.cur_block:self.next_block]
        cols.copy_(torch.where(self.in_progress[:, None], torch.full_like(cols, value), cols))
        lo, hi = self._dirty if self._dirty else (self.cur_block, self.next_block)
        self._dirty = (min(lo, self.cur_block), max(hi, self.next_block))

    def increase_block(self):
        self._set_block(1.0)
        self.cur_block = self.next_block
        self.next_block += self.block_size
        if self.model.encoding_dim - self.next_block < self.block_size:
            self.next_block = self.model.encoding_dim

    def update_mask(self):
        if self.train() and self.iteration < self.block_iterations and self._in_progress_any:
            alpha = min(1., float(2 * (self.iteration % self.block_iterations)) / self.block_iterations)
            self._set_block(alpha)

    def init_mask(self):
        return torch.ones(self.res ** self.mask_dim, self.model.encoding_dim)

    def blur(self, lo=0, hi=None):
        """get_mask_ for the columns lo:hi of the mask: (res^3, hi - lo), the k^3 box blur with replicate padding"""
        cols = self.mask[:, lo:hi].contiguous()
        out = _box_sum(cols.view(self.res, self.res, self.res, cols.shape[1]), self.k) * (1.0 / self.k ** 3)
        return out.view(-1, cols.shape[1])

    def get_mask(self):
        """the blurred grid (res^3, 515), cached; after a change of the block in progress only its columns are blurred again and
        written into the cached tensor in place"""
        with torch.no_grad():
            if self.mask_ is None or self.mask_.device != self.mask.device:
                self.mask_ = self.blur()
            elif self._dirty:
                lo, hi = self._dirty
                self.mask_[:, lo:hi] = self.blur(lo, hi)
            self._dirty = None
        return self.mask_

    @property
    def k_active(self):
        """every column of the grid from here on is zero: the block in progress ends at next_block (a loaded checkpoint may have
        opened more than this object's counters know)"""
        return max(self.next_block, self._loaded_open)

    def device_grid(self, device):
        """Mask(blurred grid on the device, k_active, res, centre_scale): what the spatial kernels take"""
        device = torch.device(device)
        if self.mask.device.type != device.type or (device.index is not None and self.mask.device.index != device.index):
            raise ValueError(f'the controller is on {self.mask.device}, the grid of points on {device}: move it with .to()')
        return Mask(self.get_mask(), self.k_active, self.res, self.centre_scale_host())

    # ---- cells of points ----
    def flat_inds(self, indices, alphas):
        mask_inds, mask_alphas = [], []
        for i in range(2 ** self.mask_dim):
            select = ('{' + f'0:0{self.mask_dim}b' + '}').format(i)
            cur_ind, cur_alpha = 0, 1
            for j, (s, inds, alpha) in enumerate(zip(select, indices, alphas)):
                s = int(s)
                cur_ind += inds[s] * self.res ** j
                cur_alpha *= alpha[s]
            mask_inds.append(cur_ind.long())
            mask_alphas.append(cur_alpha)
        return torch.stack(mask_inds, 1), torch.stack(mask_alphas, 1)

    def cells(self, x):
        """(inds (N, 8), alphas (N, 8)) of interpolate_ for points x (N, 3): the fp32 expressions the kernels restate"""
        x = self.scale(x)
        x_ = ((x + 1) / 2) * max((self.res - 2), 1) + .5
        inds = [(torch.floor(x_[:, i]), torch.ceil(x_[:, i] + 1e-6)) for i in range(self.mask_dim)]
        alphas = [(inds[i][1] - x_[:, i], x_[:, i] - inds[i][0]) for i in range(self.mask_dim)]
        return self.flat_inds(inds, alphas)

    def interpolate(self, x):
        """the reference's gather + einsum, (N, 515): for tests and the composed path, it builds the (N, 8, 515) tensor"""
        with torch.no_grad():
            inds, alphas = self.stash = self.cells(x)
            mask = self.get_mask()[inds].to(alphas)
            return torch.einsum('ndf,nd->nf', mask, alphas)

    def note_grid(self, times, ys, xs):
        """flow_fields: the grid of points just evaluated; stash_iteration computes its cells when it needs them"""
        self._last_grid, self._last_list = (times, ys, xs), None
        self.stash = (None, None)

    def note_poses(self, x):
        """flow_at: the pose list (N, 3) just evaluated, as note_grid"""
        self._last_grid, self._last_list = None, x.detach().reshape(-1, 3)
        self.stash = (None, None)

    def _last_poses(self):
        if self._last_list is not None:
            return self._last_list
        if self._last_grid is None:
            raise RuntimeError('stash_iteration before any evaluation: no points to attribute the loss to')
        gt, gh, gw = torch.meshgrid(*self._last_grid, indexing='ij')
        return torch.stack((gt, gh, gw), dim=-1).view(-1, 3)

    def __call__(self, x, **kwargs):
        """progressive_controller.py:670-680 on flow_at: the per-point mask is interpolated inside the kernels from this controller's blurred
        grid, or from an `override_mask` grid (res^3, 515); `get_mask` among the keywords returns (out, the interpolated mask (..., 515));
        `pose_grad=True` is flow_at's.  `mask_by` (a mask taken at other points) and `expand_by` (a function of the mask) are not built"""
        for key in ('mask_by', 'expand_by'):
            if key in kwargs:
                raise NotImplementedError(f'StashedSpatialController: the `{key}` keyword is not supported: the mask is interpolated inside '
                                          f'the kernels at the poses themselves')
        return flow_at(self, x, 1.0, override_mask=kwargs.get('override_mask'), get_mask='get_mask' in kwargs,
                       pose_grad=kwargs.get('pose_grad', False), jacobian=kwargs.get('jacobian'))

    # ---- checkpoints ----
    def load_mask(self):
        super().load_mask()
        self.mask = self.mask.to(self.mask_stashed.device)
        self.mask_ = None
        self._dirty = None
        self._in_progress_any = self._any(self.in_progress)
        self._loaded_open = min(self.encoding_dim, int(torch.ceil(self.mask_stashed.max()).item()))

    def __init__(self, model, res, block_iterations=20, epsilon=1e-3, mask_dim=None):
        self.res = max(res, 3)
        if mask_dim is None:
            mask_dim = model.domain_dim
        if mask_dim != 3 or model.domain_dim != 3:
            raise ValueError(f'StashedSpatialController: mask_dim == domain_dim == 3 only (got {mask_dim}, {model.domain_dim})')
        self.mask_dim = mask_dim
        super().__init__(model)
        device = next(model.parameters()).device
        self.mask = self.mask.to(device)
        self.mask_stashed = self.mask_stashed.to(device)
        in_progress = torch.ones(*self.mask.shape[:-1], dtype=torch.bool, device=device)
        self.register_buffer('in_progress', in_progress)
        self.block_size = model.domain_dim * 2
        num_blocks = (self.encoding_dim - self.block_size) // self.block_size
        self.mask[:, self.block_size:] = 0
        self.mask_ = None
        self._dirty = None
        self._in_progress_any = True
        self._loaded_open = 0
        self._last_grid = self._last_list = None
        self.cur_block = self.block_size
        self.next_block = self.block_size * 2
        self.block_iterations = block_iterations
        self.progress_iterations = self.block_iterations * num_blocks
        self.trigger = False
        self.epsilon_ = epsilon
        self.k = 5 if self.mask.shape[0] > 100 else 3
        self.stash = None, None
        self.register_buffer('log_buffer', torch.zeros(self.mask.shape[0], dtype=torch.float, device=device))
        self.register_buffer('log_counter', torch.zeros(self.mask.shape[0], dtype=torch.float, device=device))
        self.center_scale = torch.zeros(2, 1, self.domain_dim)      # host: six floats, passed to the kernels by value
        self.center_scale[1, :] = 1
        self.scale = self.scale_dummy
