"""The controllers of the progressive encoding (video-interpolation/progressive_controller.py:14-158): a module around a
progressive model (`sin_inn_amd.flownet.PRBFModel` / `PFFModel` / `PUFFModel`) that owns the per-feature mask and opens it
block by block as training goes on, as video-interpolation/main.py:136-143 wraps every `is_progressive` network.

    ProgressiveEncoderController   progressive_controller.py:14-92
    LinearController               progressive_controller.py:95-132
    LinearControllerEarly          progressive_controller.py:135-158   (the one main.py uses unless --spatially-adaptive is given)

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
Calling a controller on a pose list raises like the models do (`flow_fields` evaluates a controller on a grid).

Out of scope: StashedSpatialController (`--spatially-adaptive`: a per-point mask interpolated from a 50^3 grid),
FixedSpatialController, AdaptiveController.
"""
import torch
import torch.nn as nn

from .flownet import last_open


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
        if 'override_mask' in kwargs and kwargs['override_mask'] is not None:
            override_mask = kwargs['override_mask']
        else:
            override_mask = self.mask
        out = self.model(x, override_mask=override_mask)
        if 'get_mask' in kwargs:
            return out, override_mask
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
        """(mask on `device`, k_active); uploads only if the host mask changed since the last call for this device"""
        device = torch.device(device)
        hit = self._device_masks.get(device)
        if hit is None or not torch.equal(hit[0], self.mask):
            host = self.mask.detach().to(torch.float32).contiguous()
            assert host.dim() == 1 and host.numel() == self.encoding_dim, 'a global mask of encoding_dim values'
            snapshot = host.clone()
            hit = (snapshot, snapshot.pin_memory().to(device, non_blocking=True), last_open(snapshot))
            self._device_masks[device] = hit
            self.uploads += 1
        return hit[1], hit[2]

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
