"""Frame synthesis from a fitted pair of flows: what turns two frames and their two flows into the frames between them.

    synthesize(frame1, frame2, flow12, flow21, taus)   the fused operator, csrc/flowsynth.hip: two launches whatever len(taus) is
    composed(frame1, frame2, flow12, flow21, taus)     the same definition from the existing operators and torch: its A/B partner

The definition, for frames I0, I1 (B, C, H, W), flows F01, F10 (B, 2, H, W) in pixels and times tau (K,) in [0, 1]:

    Z0 = -20 mean_c |I0 - warp(I1, F01)|,  Z1 = -20 mean_c |I1 - warp(I0, F10)|     the trainer's metric (trainer.py:61-68); warp is
                                                                                    Resample2d, `functional.flow_warp_l1`
    S0 = softmax-splat(I0, tau_k F01, Z0), S1 = softmax-splat(I1, (1 - tau_k) F10, Z1)      FunctionSoftsplat(.., 'softmax');
                                                                                    N0, N1: the splatted exp(Z) before its guard
    a0 = (1 - tau_k) (N0 != 0),  a1 = tau_k (N1 != 0)
    out[:, k] = (a0 S0 + a1 S1) / (a0 + a1)   where a0 + a1 != 0,   (1 - tau_k) I0 + tau_k I1 elsewhere (both splats empty)

-0.0 counts as zero.  Resample2d divides by (W - 1, H - 1): on an axis of length 1 its sampling coordinate is infinite, the sample
lies outside the frame and the warped value is 0 there.  The operator is for inference and has no gradient.
"""
import ctypes as C

import torch

from . import _lib
from .ops import _stream, ptr

check = _lib.check
MAX_TIMES = 64          # FS_MAX_K of csrc/flowsynth.hip


def _host_taus(taus):
    """the times as a list of Python floats (validated on the host, where a sequence or a host tensor already is)"""
    if torch.is_tensor(taus):
        assert taus.dim() == 1, 'taus: a sequence or a 1-D tensor'
        values = taus.detach().cpu().to(torch.float64).tolist()
    else:
        values = [float(t) for t in taus]
    if not values:
        raise ValueError('flowsynth: taus is empty')
    if len(values) > MAX_TIMES:
        raise ValueError(f'flowsynth: {len(values)} times in one call, at most {MAX_TIMES}')
    if not all(0.0 <= t <= 1.0 for t in values):
        raise ValueError(f'flowsynth: every tau must lie in the range [0, 1], got {values}')
    return values


def _check_inputs(who, frame1, frame2, flow12, flow21):
    for t in (frame1, frame2, flow12, flow21):
        if t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f'flowsynth.{who} is an inference operator and has no gradient: detach its inputs '
                               '(or call it under torch.no_grad())')
    b, c, h, w = frame1.shape
    assert frame2.shape == frame1.shape, f'flowsynth.{who}: the two frames differ in shape'
    assert tuple(flow12.shape) == (b, 2, h, w) and tuple(flow21.shape) == (b, 2, h, w), f'flowsynth.{who}: flows are (B, 2, H, W)'
    return b, c, h, w


def _gpu32(t):
    if not t.is_cuda:
        raise NotImplementedError('sin-inn_amd flow-synthesis operators run on the GPU only (got a CPU tensor)')
    assert t.dtype == torch.float32, 'fp32 tensors expected'
    return t.detach()


def _planes(flow):
    """a (B, 2, H, W) flow the kernel can read: the channel-slice views `flow_fields` returns are copied, a contiguous one is not"""
    return flow if flow.is_contiguous() else flow.contiguous()


def workspace_floats(b, k, c, h, w):
    return int(_lib.lib().sininn_flow_synth_workspace(b, k, c, h, w))


def synthesize(frame1, frame2, flow12, flow21, taus, *, out=None, u8=False, workspace=None):
    """The frames at `taus` between frame1 (tau = 0) and frame2 (tau = 1): (B, K, C, H, W) fp32, and with u8=True also the same
    frames as bytes, clamp(round(255 * out), 0, 255).  `flow12` carries frame1 onto frame2, `flow21` the reverse, in pixels, channel 0
    = x: what `flow_fields` returns.  `taus`: a sequence, or a 1-D tensor on the host or the device.  `workspace`: an fp32 device
    buffer of at least `workspace_floats(B, K, C, H, W)` values (allocated here otherwise); it is zeroed inside the call."""
    b, c, h, w = _check_inputs('synthesize', frame1, frame2, flow12, flow21)
    values = _host_taus(taus)
    frame1, frame2 = _gpu32(frame1).contiguous(), _gpu32(frame2).contiguous()
    flow12, flow21 = _planes(_gpu32(flow12)), _planes(_gpu32(flow21))
    k = len(values)
    dev = frame1.device
    if torch.is_tensor(taus) and taus.is_cuda and taus.dtype == torch.float32:
        tau = taus.detach().contiguous()
    else:
        tau = torch.tensor(values, dtype=torch.float32, device=dev)
    need = workspace_floats(b, k, c, h, w)
    if workspace is None:
        workspace = torch.empty(need, device=dev, dtype=torch.float32)
    assert workspace.is_cuda and workspace.dtype == torch.float32 and workspace.is_contiguous(), 'workspace: contiguous fp32 on the device'
    if out is None:
        out = torch.empty((b, k, c, h, w), device=dev, dtype=torch.float32)
    assert tuple(out.shape) == (b, k, c, h, w) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
    bytes_ = torch.empty((b, k, c, h, w), device=dev, dtype=torch.uint8) if u8 else None
    check(_lib.lib().sininn_flow_synth(ptr(frame1), ptr(frame2), ptr(flow12), ptr(flow21), ptr(tau), b, k, c, h, w, ptr(workspace),
                                       workspace.numel(), ptr(out), C.c_void_p(bytes_.data_ptr()) if u8 else None, _stream()))
    return (out, bytes_) if u8 else out


def compose_from(frame1, frame2, flow12, flow21, values, metric, softsplat_sum):
    """The definition, operator by operator, in the dtype and on the device of the frames.  `metric(target, img, flow)` is
    mean_c |target - warp(img, flow)| as (B, 1, H, W) and `softsplat_sum(inp, flow)` the summation splat: `composed` passes this
    package's kernels, the tests the float64 functions of `oracle`."""
    tau = torch.tensor(values, dtype=frame1.dtype, device=frame1.device)
    z0, z1 = -20 * metric(frame1, frame2, flow12), -20 * metric(frame2, frame1, flow21)
    in0 = torch.cat([frame1 * z0.exp(), z0.exp()], 1)
    in1 = torch.cat([frame2 * z1.exp(), z1.exp()], 1)
    frames = []
    for k in range(len(values)):
        t, s = tau[k], 1 - tau[k]
        acc0, acc1 = softsplat_sum(in0, t * flow12), softsplat_sum(in1, s * flow21)
        n0, n1 = acc0[:, -1:], acc1[:, -1:]
        s0 = acc0[:, :-1] / torch.where(n0 == 0.0, torch.ones_like(n0), n0)
        s1 = acc1[:, :-1] / torch.where(n1 == 0.0, torch.ones_like(n1), n1)
        a0, a1 = s * (n0 != 0).to(frame1.dtype), t * (n1 != 0).to(frame1.dtype)
        den = a0 + a1
        blend = (a0 * s0 + a1 * s1) / torch.where(den != 0, den, torch.ones_like(den))
        frames.append(torch.where(den != 0, blend, s * frame1 + t * frame2))
    return torch.stack(frames, 1)


def composed(frame1, frame2, flow12, flow21, taus):
    """`synthesize` restated with the existing operators: `functional.flow_warp_l1` (warp and metric, as the trainer calls it),
    `flowloss`'s summation splat (the scatter FunctionSoftsplat(.., 'softmax') runs, normalised as it normalises) and torch
    arithmetic: about sixteen launches per time.  Its float64 form on the CPU is `tests/flowsynth_refs.composed64`, which passes
    `compose_from` the functions of `oracle`."""
    b, c, h, w = _check_inputs('composed', frame1, frame2, flow12, flow21)
    values = _host_taus(taus)
    from .flowloss import _FunctionSoftsplat
    from .functional import flow_warp_l1

    def metric(target, img, flow):
        if h < 2 or w < 2:                  # flow_warp_l1 refuses an axis of length 1: the warped frame is 0 there (see above)
            return target.abs().mean(1, keepdim=True)
        return flow_warp_l1(img, flow, target)[1]

    with torch.no_grad():
        frame1, frame2 = _gpu32(frame1).contiguous(), _gpu32(frame2).contiguous()
        flow12, flow21 = _gpu32(flow12).contiguous(), _gpu32(flow21).contiguous()
        return compose_from(frame1, frame2, flow12, flow21, values, metric, _FunctionSoftsplat.apply)
