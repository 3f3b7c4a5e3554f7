"""Fused optimisers on flat parameter buffers.

FusedAdam, for the INN parameters (replaces torch.optim.Adam of lit_wrapper.py:131-138).
All parameters are re-homed into ONE flat fp32 buffer (and their gradients into another) so that
  * the optimiser step is a single HIP launch over 3.7 M elements (p, g, m, v streams), and
  * data-parallel training needs a single RCCL all-reduce of the flat gradient per step.
Arithmetic == torch.optim.Adam (L2 weight decay added to the gradient, bias corrections, eps outside
the sqrt); parity is tested against torch.optim.Adam itself.

FusedLAMB, for the flow-field networks (replaces apex.optimizers.FusedLAMB of video-interpolation/trainer.py:134-135).
The same flat buffers with every tensor on a 16-byte boundary, a chunk table built once on the host (`lamb_layout`), and five
small launches per param group and step (csrc/lamb.hip; the formulas are in include/sininn.h, the plan in DESIGN 15).  The global
gradient norm, the clip factor and the per-tensor trust ratios never leave the device.  apex is the specification, restated; parity
with apex's binary is not pinned.
"""
import torch

from . import _lib, ops
from .modules import bump_weights_epoch, join_side_streams

LAMB_CHUNK = 4096


def _flat_offsets(numels, align):
    """start offset of every tensor (each a multiple of `align`) and the buffer length, rounded up to 4 elements"""
    offs, off = [], 0
    for k in numels:
        off = (off + align - 1) // align * align
        offs.append(off)
        off += k
    return offs, (off + 3) // 4 * 4


def lamb_layout(numels, chunk=LAMB_CHUNK):
    """Host-only layout of FusedLAMB's flat buffers for tensors of `numels` elements: (tensor offsets, padded length, chunk table).
    Every offset is a multiple of 4 elements; the chunk table lists (tensor, begin, len) with len <= chunk, in order, tiling each
    tensor exactly once, so no chunk crosses a tensor or touches the padding between tensors."""
    assert chunk > 0 and chunk % 4 == 0, 'the chunk size must be a positive multiple of 4'
    assert len(numels) > 0 and all(int(k) > 0 for k in numels), 'every tensor needs at least one element'
    offs, npad = _flat_offsets([int(k) for k in numels], 4)
    chunks = [(t, off + b, min(chunk, k - b)) for t, (off, k) in enumerate(zip(offs, numels)) for b in range(0, int(k), chunk)]
    return offs, npad, chunks


class _FlatOptimizer(torch.optim.Optimizer):
    """Parameters and gradients of every param group re-homed into one flat fp32 buffer each; m and v beside them."""
    _ALIGN = 1                              # elements; FusedAdam packs tensors back to back, FusedLAMB on 16-byte boundaries

    def _build_flat(self):
        name = type(self).__name__
        self._flat = []
        for group in self.param_groups:
            ps = [p for p in group['params'] if p.requires_grad]
            assert ps, 'empty parameter group'
            dev = ps[0].device
            if dev.type != 'cuda':
                raise NotImplementedError(f'{name} runs on the GPU only: move the module to cuda first')
            offs, npad = _flat_offsets([p.numel() for p in ps], self._ALIGN)
            flat_p = torch.zeros(npad, device=dev, dtype=torch.float32)
            flat_g = torch.zeros(npad, device=dev, dtype=torch.float32)
            for p, off in zip(ps, offs):
                assert p.dtype == torch.float32 and p.device == dev
                k = p.numel()
                flat_p[off:off + k].copy_(p.detach().reshape(-1))
                had_grad = p.grad
                p.data = flat_p[off:off + k].view(p.shape)             # parameter storage -> flat buffer
                p.grad = flat_g[off:off + k].view(p.shape)             # gradient storage  -> flat buffer
                if had_grad is not None:
                    p.grad.copy_(had_grad)
            self._flat.append(dict(p=flat_p, g=flat_g, m=torch.zeros_like(flat_p), v=torch.zeros_like(flat_p),
                                   n=sum(p.numel() for p in ps), step=0, params=ps, offsets=offs))
        bump_weights_epoch()

    # the flat gradient buffer must survive zero_grad (views would be lost with set_to_none=True)
    def zero_grad(self, set_to_none=False):
        join_side_streams()
        for fl in self._flat:
            fl['g'].zero_()

    def flat_grads(self):
        join_side_streams()                 # weight-gradient kernels run on a side stream
        return [fl['g'] for fl in self._flat]

    def flat_grads_nojoin(self):
        """the flat gradient buffers, no stream join (inside a graph capture the caller has joined already)"""
        return [fl['g'] for fl in self._flat]

    def flat_grad_buffers(self):
        """The flat gradient buffers and the stream a collective over them has to be ordered behind.  That is the weight-gradient
        stream ALONE (no join; dist.allreduce_sum_(..., after=stream)) only while EVERY parameter of the buffers is an
        executor-owned conv parameter, i.e. all writes into the buffers are issued on that stream (modules._grad_buf tags them).
        A model with any other trainable parameter -- a torch-native layer whose gradient autograd writes on the main or the
        second pass stream -- gets (buffers, None) after a join of the streams: the collective is then ordered behind the
        caller's stream, which has waited for everything."""
        from .modules import side_stream_if_any
        bufs = [fl['g'] for fl in self._flat]
        if not self.__dict__.get('_all_executor_owned', False):
            self.__dict__['_all_executor_owned'] = all(p.__dict__.get('_sininn_executor_grad', False)
                                                       for fl in self._flat for p in fl['params'])
        if not self._all_executor_owned:
            join_side_streams()
            return bufs, None
        return bufs, side_stream_if_any(bufs[0].device)

    def flat_params(self):
        return [fl['p'] for fl in self._flat]

    def _check_grads_in_flat(self, fl):
        lo, hi = fl['g'].data_ptr(), fl['g'].data_ptr() + fl['g'].numel() * 4
        for p in fl['params']:
            if p.grad is None or not (lo <= p.grad.data_ptr() < hi):
                raise RuntimeError(f'{type(self).__name__}: a parameter gradient left the flat buffer '
                                   '(use this optimizer\'s zero_grad(), not set_to_none)')

    def state_dict(self):
        return {'flat': [dict(m=fl['m'].clone(), v=fl['v'].clone(), step=fl['step']) for fl in self._flat],
                'param_groups': [{k: v for k, v in g.items() if k != 'params'} for g in self.param_groups]}

    def load_state_dict(self, sd):
        for fl, s in zip(self._flat, sd['flat']):
            fl['m'].copy_(s['m']); fl['v'].copy_(s['v']); fl['step'] = int(s['step'])
        for g, s in zip(self.param_groups, sd['param_groups']):
            g.update(s)


class FusedAdam(_FlatOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._build_flat()

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        loss = closure() if closure is not None else None
        join_side_streams()
        for group, fl in zip(self.param_groups, self._flat):
            self._check_grads_in_flat(fl)
            fl['step'] += 1
            b1, b2 = group['betas']
            ops.adam_step(fl['p'], fl['g'], fl['m'], fl['v'], group['lr'], b1, b2, group['eps'],
                          group['weight_decay'], fl['step'], grad_scale)
        bump_weights_epoch()
        return loss


class FusedLAMB(_FlatOptimizer):
    """apex.optimizers.FusedLAMB's constructor and arithmetic (include/sininn.h has the formula block) on FusedAdam's surface.
    The gradient buffer is left unchanged by step() (apex overwrites the gradients with the update)."""
    _ALIGN = 4

    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, amsgrad=False,
                 adam_w_mode=True, grad_averaging=True, max_grad_norm=1.0, use_nvlamb=False):
        if amsgrad:
            raise RuntimeError('FusedLAMB does not support the AMSGrad variant.')
        defaults = dict(lr=lr, bias_correction=bias_correction, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                        grad_averaging=grad_averaging, max_grad_norm=max_grad_norm)
        super().__init__(params, defaults)
        self.adam_w_mode = 1 if adam_w_mode else 0
        self.use_nvlamb = use_nvlamb
        self._build_flat()
        dev = self._flat[0]['p'].device
        assert all(fl['p'].device == dev for fl in self._flat), 'FusedLAMB: all param groups must live on one device'
        self._norm_slots = torch.zeros(len(self._flat), device=dev, dtype=torch.float32)
        for gi, fl in enumerate(self._flat):
            offs, npad, chunks = lamb_layout([p.numel() for p in fl['params']])
            assert offs == fl['offsets'] and npad == fl['p'].numel()
            nt = len(offs)
            fl['u'] = torch.zeros_like(fl['p'])
            fl['chunks'] = torch.tensor(chunks, dtype=torch.int64).to(dev)                 # uploaded once
            fl['toff'] = torch.tensor(offs + [npad], dtype=torch.int64).to(dev)
            nbytes = ops.lamb_workspace_bytes(len(chunks), nt)
            fl['ws'] = torch.zeros(nbytes // 4, device=dev, dtype=torch.float32)
            fl['n_tensors'] = nt
            a = _lib.LambArgs(n=npad, n_chunks=len(chunks), n_tensors=nt, group=gi, n_groups=len(self._flat),
                              workspace_bytes=nbytes)
            a.p, a.g, a.m, a.v, a.u = (fl[k].data_ptr() for k in 'pgmvu')
            a.chunks, a.tensor_offsets = fl['chunks'].data_ptr(), fl['toff'].data_ptr()
            a.norm_slots, a.workspace = self._norm_slots.data_ptr(), fl['ws'].data_ptr()
            fl['args'] = a

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        loss = closure() if closure is not None else None
        join_side_streams()
        for group, fl in zip(self.param_groups, self._flat):
            self._check_grads_in_flat(fl)
            fl['step'] += 1
            a = fl['args']
            a.lr, (a.beta1, a.beta2), a.eps, a.weight_decay = group['lr'], group['betas'], group['eps'], group['weight_decay']
            a.max_grad_norm, a.grad_scale, a.step = group['max_grad_norm'], grad_scale, fl['step']
            a.bias_correction, a.grad_averaging = int(bool(group['bias_correction'])), int(bool(group['grad_averaging']))
            a.adam_w_mode, a.use_nvlamb = self.adam_w_mode, int(bool(self.use_nvlamb))
            ops.lamb_grad_norm(a)           # the global norm spans all groups: every slot is written before any stage 1
        for fl in self._flat:
            ops.lamb_step(fl['args'])
        bump_weights_epoch()
        return loss

    def last_trust_ratios(self):
        """the per-tensor ratios (lr * |p| / |u|, or lr) the last step applied, one device tensor per param group; diagnostic"""
        return [fl['ws'][:fl['n_tensors']] for fl in self._flat]
