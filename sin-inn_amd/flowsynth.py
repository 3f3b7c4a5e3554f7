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

    gather(frame1, frame2, flows, slots, taus)            the second synthesis rule, csrc/flowgather.hip: one launch
    gather_composed(frame1, frame2, flows, slots, taus)   the same definition from torch ops, on any device, fp32 or fp64
    gather_slots(times, taus, dt, back)                   host logic: the time stamps to evaluate the network at, and the slot table

`gather` takes the flows at the in-between time s = t0 + tau dt, where they live on the grid of the frame being synthesized, and reads
both source frames through a backward warp.  `flows` is a (T', 4, H, W) tensor in `flow_fields`' layout (channels 0-1 forward, 2-3
backward); per output frame (b, k) the slot table names the time slice and channel pair of G0 (toward the previous frame) and of G1
(toward the next one) and the coefficients c0, c1:

    q0 = p + c0 G0(p),  q1 = p + c1 G1(p);    (W0, n0) = sample(I0, q0),  (W1, n1) = sample(I1, q1)
    a0 = 1 - tau, a1 = tau,  L = a0 I0(p) + a1 I1(p);    out = (a0 W0 + a1 W1 + e L) / (a0 n0 + a1 n1 + e),  e = 2^-10

`sample` is the bilinear gather with pixel centres at integers (not Resample2d's geometry): a tap outside the frame adds 0 to W and to
n, the sum of the weights inside.  The regular slot is G1 = fw(s), c1 = 1 - tau, G0 = bw(s - dt), c0 = tau; where s - dt lies before
the clip's first frame, and throughout under back='reverse', G0 = fw(s) with c0 = -tau (constant velocity).  No atomics and no
accumulator: equal inputs give equal bits.

    gather(.., flow_grad=True), gather_composed(.., flow_grad=True)    the result carries a gradient to `flows`
    gather_reduce_list(slots, slices)                                  host logic: which rows add to which slice, in which order

Without the keyword both are inference operators and refuse inputs that require grad.  With it, `gather` differentiates with respect to
the flows -- and nothing else: not the frames, tau or the coefficients; once -- through the backward kernels of csrc/flowgather.hip:

    dG0 = c0 a0 / D  sum_c g_c (grad_q W0_c - out_c grad_q n0),   dG1 likewise;   D = a0 n0 + a1 n1 + e

grad_q is the derivative of the bilinear interpolant of the zero-padded plane in the cell floor(q) (on a cell border the right-hand
derivative, what autograd gives through `gather_from`); a sample whose coordinate is not finite, or 1e9 or more in size, has gradient 0.
Rows that name the same slice and channel pair are summed in ascending b K + k, dG0 before dG1, without atomics.

    gather(.., visible=(m1, m2)), gather_composed(.., visible=(m1, m2))    the occlusion-aware rule

m1 is 1 where a pixel of frame 1 is visible in frame 2, m2 the same for frame 2 in frame 1 (the trainer's mask1, mask2).  With
S(X, q) the taps and weights of W (a tap outside the frame adds 0):

    o0 = S(1 - m1, q0), o1 = S(1 - m2, q1);   v0 = 1 - o1, v1 = 1 - o0;   out = (a0 v0 W0 + a1 v1 W1 + e L) / (a0 v0 n0 + a1 v1 n1 + e)

A sample is trusted unless the surface the other sample found is hidden in its frame.  All-ones masks give the plain rule's bits; where
both v are 0 the result is L.  One launch; no gradient, and not at a point list.

    quality(pred, target)            PSNR and mean SSIM per frame, the fused operator of csrc/framequality.hip
    quality_composed(pred, target)   the same definition from torch ops, on any device, fp32 or fp64: its A/B partner and reference

For frames p, t (B, C, H, W) with values in [0, 1] (data range 1):

    mse = mean (p - t)^2,   psnr = 10 log10(1 / mse)  (+inf where mse == 0)
    ssim = the mean over channels and all valid 11 x 11 windows of ((2 mu_p mu_t + C1)(2 s_pt + C2)) / ((mu_p^2 + mu_t^2 + C1)(s_p + s_t + C2))

with the Gaussian window of sigma 1.5, C1 = 0.01^2, C2 = 0.03^2 (Wang et al. 2004).  `quantize=True` measures the frames as the bytes a
PNG holds: both inputs go through `synthesize`'s u8 rule first, clamp(round-half-even(255 v), 0, 255).
"""
import collections
import ctypes as C
import math
import struct

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


def _refuse_grad(who, tensors, flow_grad=False, hint=''):
    """the refusal of inputs that require grad: every input of an inference operator, the frames under flow_grad=True"""
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        if flow_grad:
            raise RuntimeError(f'flowsynth.{who}(.., flow_grad=True) has a gradient with respect to the flows only: detach the frames')
        raise RuntimeError(f'flowsynth.{who} is an inference operator and has no gradient: detach its inputs '
                           f'(or call it under torch.no_grad(){hint})')


def _device_tau(taus, values, device):
    """the validated times as an fp32 tensor on `device`: `taus` itself where it already is one"""
    if torch.is_tensor(taus) and taus.is_cuda and taus.dtype == torch.float32:
        return taus.detach().contiguous()
    return torch.tensor(values, dtype=torch.float32, device=device)


def _check_inputs(who, frame1, frame2, flow12, flow21):
    _refuse_grad(who, (frame1, frame2, flow12, flow21))
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
    tau = _device_tau(taus, values, dev)
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


# ---- synthesis by gathering ----

GATHER_EPS = 2.0 ** -10
SLOT_INTS = 6           # FG_SLOT_INTS of csrc/flowgather.hip: idx0, idx1, ch0, ch1, bits of c0, bits of c1
BWD_IN_PLACE = None     # the backward path of `gather(.., flow_grad=True)`: None: one launch where the table's targets are distinct, else
                        # two; True / False force a path (True needs distinct targets).  Both give the same bits
K_LOOP = False          # the launch shape of `gather`: one lane per (b, k, y, x); True: a lane walks the K times of its pixel
DeviceSlots = collections.namedtuple('DeviceSlots', 'table slices')     # a validated table on the device; slices: the T' it needs


def _f32(v):
    """v rounded to fp32, as a Python float"""
    return struct.unpack('<f', struct.pack('<f', v))[0]


def _f32_bits(v):
    return struct.unpack('<i', struct.pack('<f', v))[0]


def slot_coefficients(slots):
    """(c0, c1) of a host slot table as an fp32 tensor (B, K, 2)"""
    return slots[..., 4:].contiguous().view(torch.float32)


def gather_slots(times, taus, dt, back='network', first=-1.0):
    """Where to evaluate the network for `gather`, and what to read from the result.  `times`: the frame-1 time stamps of the batch's
    pairs (B values; a sequence or a tensor), `taus`: K values in [0, 1], `dt`: the spacing of the clip's times, `first`: the time of
    the clip's first frame.  Returns (stamps, slots):

        stamps   Python floats, each an fp32 value: first s_{b,k} = times[b] + taus[k] dt in (b, k) order -- slice b K + k --, then,
                 under back='network', s_{b,k} - dt in the same order for every (b, k) where that is not before `first`
        slots    the table, a host int32 tensor (B, K, 6): idx0, idx1, ch0, ch1 and the bits of c0, c1 (`slot_coefficients`).
                 G1 = fw(s): idx1 = b K + k, ch1 = 0, c1 = 1 - tau.  G0 = bw(s - dt): idx0 the slice of s - dt, ch0 = 2, c0 = tau.
                 Where s - dt < first (pairs of the clip's first frame, tau < 1), and everywhere under back='reverse':
                 G0 = fw(s), idx0 = idx1, ch0 = 0, c0 = -tau.

    `s - dt < first` is decided with a slack of dt / 1000, which covers the fp32 rounding of the clip's times.  Pure host logic."""
    if back not in ('network', 'reverse'):
        raise ValueError(f"flowsynth.gather_slots: back is 'network' or 'reverse', got {back!r}")
    values = _host_taus(taus)
    t0s = [float(t) for t in (times.detach().cpu().to(torch.float64).tolist() if torch.is_tensor(times) else times)]
    dt = float(dt)
    if not t0s or not dt > 0:
        raise ValueError('flowsynth.gather_slots: at least one pair, and dt > 0')
    k = len(values)
    stamps = [_f32(t0 + tau * dt) for t0 in t0s for tau in values]
    rows = []
    for b, t0 in enumerate(t0s):
        for j, tau in enumerate(values):
            tau32 = _f32(tau)
            idx1 = b * k + j
            before = t0 + tau * dt - dt
            if back == 'network' and before >= first - 1e-3 * dt:
                idx0, ch0, c0 = len(stamps), 2, tau32
                stamps.append(_f32(before))
            else:
                idx0, ch0, c0 = idx1, 0, -tau32
            rows.append([idx0, idx1, ch0, 0, _f32_bits(c0), _f32_bits(_f32(1.0 - tau32))])
    return stamps, torch.tensor(rows, dtype=torch.int32).reshape(len(t0s), k, SLOT_INTS)


def _host_slots(who, slots, b, k):
    """the host table, validated: (B, K, 6) int32, slices >= 0, channel pairs 0 or 2, finite coefficients; returns the T' it needs"""
    if not torch.is_tensor(slots) or slots.is_cuda or slots.dtype != torch.int32 or tuple(slots.shape) != (b, k, SLOT_INTS):
        raise ValueError(f'flowsynth.{who}: slots is a host int32 tensor ({b}, {k}, {SLOT_INTS}), what gather_slots returns '
                         '(or, for gather, upload_slots)')
    if bool((slots[..., :2] < 0).any()):
        raise ValueError(f'flowsynth.{who}: a slot names a negative time slice')
    if not bool(((slots[..., 2:4] == 0) | (slots[..., 2:4] == 2)).all()):
        raise ValueError(f'flowsynth.{who}: a channel pair starts at channel 0 (forward) or 2 (backward)')
    if not bool(torch.isfinite(slot_coefficients(slots)).all()):
        raise ValueError(f'flowsynth.{who}: a slot coefficient is not finite')
    return int(slots[..., :2].max()) + 1


def upload_slots(slots, device):
    """A host table, validated and moved to `device`: what `gather` does with a host table on every call, done once"""
    if not torch.is_tensor(slots) or slots.dim() != 3:
        raise ValueError('flowsynth.upload_slots: slots is the host table of gather_slots, (B, K, 6) int32')
    b, k, _ = slots.shape
    return DeviceSlots(slots.contiguous().to(device), _host_slots('upload_slots', slots, b, k))


def _gather_inputs(who, frame1, frame2, flows, flow_grad=False):
    _refuse_grad(who, (frame1, frame2) if flow_grad else (frame1, frame2, flows), flow_grad)
    b, c, h, w = frame1.shape
    assert frame2.shape == frame1.shape, f'flowsynth.{who}: the two frames differ in shape'
    if c not in (1, 3):
        raise ValueError(f'flowsynth.{who}: frames have 1 or 3 channels (got {c})')
    assert flows.dim() == 4 and tuple(flows.shape[1:]) == (4, h, w), f'flowsynth.{who}: flows is (T, 4, H, W), the layout of flow_fields'
    return b, c, h, w


def joined_flows(flow12, flow21):
    """The (T, 4, H, W) tensor whose channel slices `flow_fields` returned, without a copy"""
    t, two, h, w = flow12.shape
    assert two == 2 and flow21.shape == flow12.shape and flow12.stride() == flow21.stride() == (4 * h * w, h * w, w, 1) \
        and flow21.data_ptr() == flow12.data_ptr() + 2 * h * w * flow12.element_size(), \
        'joined_flows: the two results of one flow_fields call, channels 0-1 and 2-3 of one (T, 4, H, W) tensor'
    return flow12.as_strided((t, 4, h, w), flow12.stride(), flow12.storage_offset())


def gather_reduce_list(slots, slices):
    """The order in which the backward pass sums the per-row gradients into d flows (`slices`, 4, H, W), from a host slot table
    (B, K, 6).  Target 2 slice + ch / 2 is one channel pair of one slice; entry 2 (b K + k) + which is dG0 (which = 0) or dG1 (1) of
    row (b, k).  Returns (list, distinct): `list` the Python ints the kernel reads -- the 2 slices + 1 begins of the targets' entries
    (the last: the number of entries), then the entries, ascending within a target (ascending b K + k, dG0 before dG1) -- and
    `distinct`: no target has more than one entry.  Pure host logic."""
    b, k, _ = slots.shape
    rows = slots.reshape(b * k, SLOT_INTS).tolist()
    per = [[] for _ in range(2 * slices)]
    for bk, (idx0, idx1, ch0, ch1, _c0, _c1) in enumerate(rows):
        for which, (idx, ch) in enumerate(((idx0, ch0), (idx1, ch1))):
            if not (0 <= idx < slices and ch in (0, 2)):
                raise ValueError(f'flowsynth.gather_reduce_list: row {bk} names slice {idx}, channel {ch}; there are {slices} slices')
            per[2 * idx + ch // 2].append(2 * bk + which)           # visited in ascending 2 bk + which
    begins, entries = [0], []
    for target in per:
        entries.extend(target)
        begins.append(len(entries))
    return begins + entries, all(len(target) <= 1 for target in per)


class _GatherFlowGrad(torch.autograd.Function):
    """`gather` with a gradient to `flows`: the forward kernel, then sininn_flow_gather_bwd on the path `BWD_IN_PLACE` names"""

    @staticmethod
    def forward(ctx, flows, frame1, frame2, host_slots, table, tau, values, k_loop):
        ctx.save_for_backward(flows, frame1, frame2, table, tau)
        ctx.host_slots = host_slots
        with torch.no_grad():
            return gather(frame1, frame2, flows, DeviceSlots(table, flows.shape[0]), values, k_loop=k_loop)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        flows, frame1, frame2, table, tau = ctx.saved_tensors
        b, c, h, w = frame1.shape
        k, t = table.shape[1], flows.shape[0]
        grad_out = _gpu32(grad_out).contiguous()
        assert tuple(grad_out.shape) == (b, k, c, h, w)
        ints, distinct = gather_reduce_list(ctx.host_slots, t)
        in_place = distinct if BWD_IN_PLACE is None else bool(BWD_IN_PLACE)
        if in_place and not distinct:
            raise ValueError('flowsynth.gather: the in-place backward needs a table whose (slice, channel pair) targets are distinct')
        dev = frame1.device
        dflows = torch.empty((t, 4, h, w), device=dev, dtype=torch.float32)
        stride = flows.stride(0) if t > 1 else 4 * h * w
        lib = _lib.lib()
        if in_place:
            rlist, n_ints, ws, n_ws = None, 0, None, 0
        else:
            rl = torch.tensor(ints, dtype=torch.int32).to(dev)
            work = torch.empty(max(int(lib.sininn_flow_gather_bwd_workspace(b, k, h, w)), 1), device=dev, dtype=torch.float32)
            rlist, n_ints, ws, n_ws = C.c_void_p(rl.data_ptr()), rl.numel(), ptr(work), work.numel()
        check(lib.sininn_flow_gather_bwd(ptr(frame1), ptr(frame2), ptr(flows), stride, C.c_void_p(table.data_ptr()), ptr(tau),
                                         ptr(grad_out), b, k, c, h, w, t, rlist, n_ints, ws, n_ws, ptr(dflows), _stream()))
        return (dflows,) + (None,) * 7


def _visible_masks(who, visible, b, h, w, flow_grad):
    """the two masks of `visible=(m1, m2)`, checked: (B, 1, H, W) each, no gradient, and not together with flow_grad=True"""
    if flow_grad:
        raise ValueError(f'flowsynth.{who}: the masked rule (visible=) has no gradient yet: flow_grad=True is the plain rule\'s')
    if not isinstance(visible, (tuple, list)) or len(visible) != 2 or not all(torch.is_tensor(m) for m in visible):
        raise ValueError(f'flowsynth.{who}: visible is a pair of masks (m1, m2), what the trainer calls mask1 and mask2')
    for m in visible:
        if tuple(m.shape) != (b, 1, h, w):
            raise ValueError(f'flowsynth.{who}: a visibility mask is ({b}, 1, {h}, {w}), one plane per pair; got {tuple(m.shape)}')
    _refuse_grad(who, visible)
    return visible


def gather(frame1, frame2, flows, slots, taus, *, visible=None, out=None, u8=False, k_loop=None, flow_grad=False):
    """The frames at `taus` between frame1 and frame2 from flows taken at the in-between times: (B, K, C, H, W) fp32, and with u8=True
    also the bytes, by `synthesize`'s rule.  `flows`: (T', 4, H, W) fp32 on the device, read in place -- any stride between time slices,
    the four channel planes of a slice contiguous.  `slots`: the host table of `gather_slots` (validated and uploaded here), or what
    `upload_slots` made of it.  `k_loop`: the launch shape (None: `K_LOOP`); both give the same bits.  One launch, no workspace.

    `flow_grad=True`: where `flows` requires grad the result carries a gradient to it (see the module text); `slots` is then the host
    table (the backward pass builds its reduce list from it), and `u8` and `out=` are not supported.

    `visible=(m1, m2)`: the occlusion-aware rule.  m1 (B, 1, H, W) is 1 where a pixel of frame1 is visible in frame2, m2 the
    same for frame2 in frame1 -- the trainer's mask1 and mask2; any float or bool values, read as fp32 numbers.  Each sample is weighed
    by 1 - S(1 - m, q) of the OTHER sample: b0 = a0 (1 - S(1 - m2, q1)), b1 = a1 (1 - S(1 - m1, q0)),
    out = (b0 W0 + b1 W1 + e L) / (b0 n0 + b1 n1 + e).  All-ones masks give the plain rule's bits.  Still one launch; no gradient."""
    b, c, h, w = _gather_inputs('gather', frame1, frame2, flows, flow_grad)
    if visible is not None:
        visible = _visible_masks('gather', visible, b, h, w, flow_grad)
    if flow_grad and (u8 or out is not None):
        raise ValueError('flowsynth.gather: flow_grad=True with u8=True or out= is not supported (bytes carry no gradient, and autograd '
                         'owns the result)')
    grad = flow_grad and flows.requires_grad and torch.is_grad_enabled()
    values = _host_taus(taus)
    k = len(values)
    if grad and isinstance(slots, DeviceSlots):
        raise ValueError('flowsynth.gather: flow_grad=True takes the host table of gather_slots (the backward pass builds its '
                         'reduce list from it)')
    frame1, frame2, data = _gpu32(frame1).contiguous(), _gpu32(frame2).contiguous(), _gpu32(flows)
    dev = frame1.device
    if not isinstance(slots, DeviceSlots):
        need, host = _host_slots('gather', slots, b, k), slots
        slots = DeviceSlots(host.contiguous().to(dev), need)
    table, need = slots
    if not (table.is_cuda and table.dtype == torch.int32 and tuple(table.shape) == (b, k, SLOT_INTS) and table.is_contiguous()):
        raise ValueError(f'flowsynth.gather: the uploaded table is not ({b}, {k}, {SLOT_INTS}) int32 on the device')
    if need > data.shape[0]:
        raise ValueError(f'flowsynth.gather: the slots name time slice {need - 1}, flows has {data.shape[0]}')
    if data.stride()[1:] != (h * w, w, 1) and data.numel() > 0:
        raise ValueError('flowsynth.gather: the four channel planes of a time slice must be contiguous (any stride between slices)')
    tau = _device_tau(taus, values, dev)
    if grad:
        return _GatherFlowGrad.apply(flows, frame1, frame2, host.contiguous().clone(), table, tau, values, k_loop)
    stride = data.stride(0) if data.shape[0] > 1 else 4 * h * w
    if out is None:
        out = torch.empty((b, k, c, h, w), device=dev, dtype=torch.float32)
    assert tuple(out.shape) == (b, k, c, h, w) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
    bytes_ = torch.empty((b, k, c, h, w), device=dev, dtype=torch.uint8) if u8 else None
    tail = (b, k, c, h, w, int(K_LOOP if k_loop is None else k_loop), ptr(out), C.c_void_p(bytes_.data_ptr()) if u8 else None, _stream())
    if visible is None:
        check(_lib.lib().sininn_flow_gather(ptr(frame1), ptr(frame2), ptr(data), stride, C.c_void_p(table.data_ptr()), ptr(tau), *tail))
    else:
        m1, m2 = (_gpu32(m.to(torch.float32)).contiguous() for m in visible)
        check(_lib.lib().sininn_flow_gather_visible(ptr(frame1), ptr(frame2), ptr(data), stride, C.c_void_p(table.data_ptr()), ptr(tau),
                                                    ptr(m1), ptr(m2), *tail))
    return (out, bytes_) if u8 else out


def _tap_walk(qx, qy, h, w, term):
    """The four taps of sample(I, q) for coordinates of any one shape: `term(weight, at)` is weight times the image at the flat offsets
    `at` = y W + x, with the channel axis where the caller keeps it.  Pixel centres at integers; a tap outside the frame adds 0 to W
    and to n; a coordinate that is not finite, or 1e9 or more in size, has no tap inside.  The four products are summed in the
    kernel's order.  Returns (W, n)."""
    ok = (qx.abs() < 1e9) & (qy.abs() < 1e9)
    qx, qy = torch.where(ok, qx, torch.zeros_like(qx)), torch.where(ok, qy, torch.zeros_like(qy))
    fx, fy = qx.floor(), qy.floor()
    x0, y0 = fx.long(), fy.long()
    wx1, wy1 = qx - fx, qy - fy
    wx0, wy0 = 1 - wx1, 1 - wy1
    total, n = None, None
    for dy, dx, wy, wx in ((0, 0, wy0, wx0), (0, 1, wy0, wx1), (1, 0, wy1, wx0), (1, 1, wy1, wx1)):
        yy, xx = y0 + dy, x0 + dx
        inside = ok & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        weight = torch.where(inside, wy * wx, torch.zeros_like(wx))
        value = term(weight, yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1))
        total = value if total is None else total + value
        n = weight if n is None else n + weight
    return total, n


def bilinear_gather(img, qx, qy):
    """sample(I, q) of the definition with torch ops: img (B, C, H, W), qx, qy (B, K, H, W) -> (W (B, K, C, H, W), n (B, K, H, W)),
    by `_tap_walk`'s rule and order of summation."""
    b, c, h, w = img.shape
    k = qx.shape[1]
    flat = img.reshape(b, 1, c, h * w).expand(b, k, c, h * w)

    def term(weight, at):
        return weight[:, :, None] * flat.gather(3, at.reshape(b, k, 1, h * w).expand(b, k, c, h * w)).reshape(b, k, c, h, w)

    return _tap_walk(qx, qy, h, w, term)


def _blend(a0, a1, w0, w1, n0, n1, h0, h1, eps, axis, weights=None):
    """out = (b0 W0 + b1 W1 + eps (a0 h0 + a1 h1)) / (b0 n0 + b1 n1 + eps): W and h carry the channels at `axis`, a, b and n have no
    such axis.  `weights`: (b0, b1), the sample weights of the masked rule; None: b = a, the plain rule"""
    b0, b1 = (a0, a1) if weights is None else weights
    c0, c1 = a0.unsqueeze(axis), a1.unsqueeze(axis)
    d0, d1 = b0.unsqueeze(axis), b1.unsqueeze(axis)
    num = (d0 * w0 + d1 * w1) + eps * (c0 * h0 + c1 * h1)
    den = (b0 * n0 + b1 * n1) + eps
    return num / den.unsqueeze(axis)


def gather_from(frame1, frame2, flows, slots, values, sample=bilinear_gather, eps=GATHER_EPS, visible=None):
    """The definition, operation by operation, in the dtype and on the device of the frames.  `sample` and `eps` are the two places a
    test swaps in something else (another geometry, no renormalisation, no guard).  `visible=(m1, m2)`: the masked rule --
    o = sample(1 - m, q) through the sample's own coordinates, v0 = 1 - o1, v1 = 1 - o0, the sample weights b = a v."""
    b, c, h, w = frame1.shape
    dt, dev = frame1.dtype, frame1.device
    flows = flows.to(device=dev, dtype=dt)
    idx = slots[..., :4].to(dev, torch.long)
    coef = slot_coefficients(slots).to(dev, dt)
    a1 = torch.tensor(values, dtype=torch.float32).to(dev, dt).view(1, -1, 1, 1)
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=dt), torch.arange(w, device=dev, dtype=dt), indexing='ij')
    pair = torch.arange(2, device=dev)

    def warped(img, which, hidden=None):
        g = flows[idx[:, :, which, None], idx[:, :, 2 + which, None] + pair]                  # (B, K, 2, H, W)
        cf = coef[:, :, which, None, None]
        qx, qy = xs + cf * g[:, :, 0], ys + cf * g[:, :, 1]
        got = sample(img, qx, qy)
        return got if hidden is None else (*got, sample(hidden, qx, qy)[0][:, :, 0])       # (W, n) and o = S(1 - m, q)

    a0 = 1 - a1
    if visible is None:
        (w0, n0), (w1, n1) = warped(frame1, 0), warped(frame2, 1)
        return _blend(a0, a1, w0, w1, n0, n1, frame1[:, None], frame2[:, None], eps, 2)
    m1, m2 = (m.to(device=dev, dtype=dt) for m in visible)
    (w0, n0, o0), (w1, n1, o1) = warped(frame1, 0, 1 - m1), warped(frame2, 1, 1 - m2)
    return _blend(a0, a1, w0, w1, n0, n1, frame1[:, None], frame2[:, None], eps, 2, weights=(a0 * (1 - o1), a1 * (1 - o0)))


def gather_composed(frame1, frame2, flows, slots, taus, *, visible=None, flow_grad=False):
    """`gather` from torch ops, on the device and in the dtype of the frames (CPU or GPU, fp32 or fp64): index arithmetic and
    `torch.gather` for the taps, a few dozen launches.  `slots` is the host table.  In fp32 it rounds where the fused operator rounds.
    `flow_grad=True`: where `flows` requires grad, `gather_from` runs with autograd on and the result carries a gradient to `flows`.
    `visible=(m1, m2)`: the masked rule, as `gather` takes it; the masks are converted to the dtype of the frames."""
    b, c, h, w = _gather_inputs('gather_composed', frame1, frame2, flows, flow_grad)
    if visible is not None:
        visible = _visible_masks('gather_composed', visible, b, h, w, flow_grad)
    values = _host_taus(taus)
    need = _host_slots('gather_composed', slots, b, len(values))
    if need > flows.shape[0]:
        raise ValueError(f'flowsynth.gather_composed: the slots name time slice {need - 1}, flows has {flows.shape[0]}')
    assert frame1.dtype in (torch.float32, torch.float64) and frame2.dtype == frame1.dtype
    if flow_grad and flows.requires_grad and torch.is_grad_enabled():
        return gather_from(frame1.detach(), frame2.detach(), flows, slots, values)
    with torch.no_grad():
        return gather_from(frame1.detach(), frame2.detach(), flows.detach(), slots, values, visible=visible)


# ---- the gather rule at a list of points ----

MAX_BLENDS = 4          # FGP_MAX_R of csrc/flowgather.hip


def _gather_at_inputs(who, frame1, frame2, flows, pix, pair, tau, rev, blend, flow_grad):
    """shapes and dtypes of the point form, checked on the host (the VALUES of the device tensors cannot be, and need not: the
    operator is safe for any); returns (b, c, h, w, s, n, blend as a list of fp32 values or None)"""
    _refuse_grad(who, (frame1, frame2) if flow_grad else (frame1, frame2, flows), flow_grad,
                 ', or pass flow_grad=True for the gradient to the flows')
    for name, t in (('pix', pix), ('tau', tau)):
        if t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f'flowsynth.{who} has no gradient with respect to {name}: detach it')
    if frame1.dim() != 4 or frame2.shape != frame1.shape:
        raise ValueError(f'flowsynth.{who}: two frames of one shape (B, C, H, W)')
    b, c, h, w = frame1.shape
    if c not in (1, 3):
        raise ValueError(f'flowsynth.{who}: frames have 1 or 3 channels (got {c})')
    if flows.dim() != 3 or flows.shape[0] not in (1, 2) or flows.shape[1] != 4:
        raise ValueError(f'flowsynth.{who}: flows is (S, 4, N) with S = 1 or 2, a stack of flow_at(.., planar=True) results; got '
                         f'{tuple(flows.shape)}')
    s, _, n = flows.shape
    if n < 1:
        raise ValueError(f'flowsynth.{who}: an empty point list')
    if tuple(pix.shape) != (n, 2) or tuple(pair.shape) != (n,) or tuple(tau.shape) != (n,):
        raise ValueError(f'flowsynth.{who}: pix is ({n}, 2), pair and tau ({n},); got {tuple(pix.shape)}, {tuple(pair.shape)}, '
                         f'{tuple(tau.shape)}')
    if pair.dtype != torch.int32:
        raise ValueError(f'flowsynth.{who}: pair is int32 (got {pair.dtype})')
    if rev is not None and (tuple(rev.shape) != (n,) or rev.dtype not in (torch.bool, torch.uint8)):
        raise ValueError(f'flowsynth.{who}: rev is ({n},) bool or uint8')
    if blend is not None:
        blend = [_f32(float(v)) for v in blend]
        if not 1 <= len(blend) <= MAX_BLENDS or not all(math.isfinite(v) for v in blend):
            raise ValueError(f'flowsynth.{who}: blend is 1 to {MAX_BLENDS} finite floats on the host (None: a1 = tau per point)')
    return b, c, h, w, s, n, blend


def _gather_at_call(entry, frame1, frame2, flows, pix, pair, tau, rev, blend, extra, result):
    b, c, h, w = frame1.shape
    s, _, n = flows.shape
    r = 1 if blend is None else len(blend)
    host = (C.c_float * r)(*blend) if blend is not None else None
    check(entry(ptr(frame1), ptr(frame2), ptr(flows), ptr(pix), C.c_void_p(pair.data_ptr()), ptr(tau),
                C.c_void_p(rev.data_ptr()) if rev is not None else None, host, *extra, r, s, n, b, c, h, w, ptr(result), _stream()))
    return result


class _GatherAtFlowGrad(torch.autograd.Function):
    """`gather_at` with a gradient to `flows`: flowgather_points_kernel, then flowgather_points_bwd_kernel"""

    @staticmethod
    def forward(ctx, flows, frame1, frame2, pix, pair, tau, rev, blend):
        flows = flows.contiguous()
        ctx.save_for_backward(flows, frame1, frame2, pix, pair, tau, rev)
        ctx.blend = blend
        r = 1 if blend is None else len(blend)
        out = torch.empty((r, flows.shape[2], frame1.shape[1]), device=frame1.device, dtype=torch.float32)
        return _gather_at_call(_lib.lib().sininn_flow_gather_at, frame1, frame2, flows, pix, pair, tau, rev, blend, (), out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        flows, frame1, frame2, pix, pair, tau, rev = ctx.saved_tensors
        grad_out = _gpu32(grad_out).contiguous()
        dflows = torch.empty_like(flows)
        _gather_at_call(_lib.lib().sininn_flow_gather_at_bwd, frame1, frame2, flows, pix, pair, tau, rev, ctx.blend, (ptr(grad_out),),
                        dflows)
        return (dflows,) + (None,) * 7


def gather_at(frame1, frame2, flows, pix, pair, tau, rev=None, *, blend=None, flow_grad=False):
    """`gather`'s rule at a list of N points: (R, N, C) fp32.  Point n lies at pix[n] = (y, x), fp32 pixel coordinates of any
    value, in pair pair[n] (int32) of the batch, at the in-between time tau[n]; everything but `blend` is on the device.

        G1 = flows[0, 0:2, n], c1 = 1 - tau[n];   G0 = flows[1, 2:4, n], c0 = tau[n] where S == 2 and not rev[n], else G0 = G1, c0 = -tau[n]
        q0 = p + c0 G0, q1 = p + c1 G1;   (W0, n0) = sample(I0[b], q0), (W1, n1) = sample(I1[b], q1), H0 = sample(I0[b], p).W, H1 likewise
        out[r, n, c] = (a0 W0 + a1 W1 + e (a0 H0 + a1 H1)) / (a0 n0 + a1 n1 + e),   a1 = blend[r], a0 = 1 - a1, e = 2^-10

    `flows`: (S, 4, N), S = 1 or 2 -- torch.stack of `flownet.flow_at(.., planar=True)` results at (s, y, x) and, for S = 2, at
    (s - dt, y, x).  `blend`: 1 to 4 host floats; None: one blend, a1 = tau[n], the interpolated frame.  A point on an integer pixel
    gets the bits `gather` gives that pixel.  Nothing in a device tensor is trusted: a pair outside [0, B) gives a row of zeros and a
    zero gradient, a coordinate that is not finite (or 1e9 or more in size) has no tap.  One launch, no workspace, no atomics.

    `flow_grad=True`: where `flows` requires grad the result carries a gradient to it, and to nothing else, by `gather`'s formulas in
    one more launch: dG1 lands in [0, 0:2], dG0 in [1, 2:4] or, where G0 = G1, is added as dG0 + dG1; the other values of the column
    are zeros; the R blends are summed in ascending r.  Equal inputs give equal bits."""
    b, c, h, w, s, n, blend = _gather_at_inputs('gather_at', frame1, frame2, flows, pix, pair, tau, rev, blend, flow_grad)
    frame1, frame2 = _gpu32(frame1).contiguous(), _gpu32(frame2).contiguous()
    pix, tau = _gpu32(pix).contiguous(), _gpu32(tau).contiguous()
    if pix.data_ptr() % 8:
        pix = pix.clone()                   # the kernel reads (y, x) as one 8-byte load
    if not pair.is_cuda or (rev is not None and not rev.is_cuda):
        raise NotImplementedError('sin-inn_amd flow-synthesis operators run on the GPU only (got a CPU tensor)')
    pair = pair.detach().contiguous()
    if rev is not None:
        rev = rev.detach().contiguous()
        rev = rev.view(torch.uint8) if rev.dtype == torch.bool else rev
    _gpu32(flows)
    if flow_grad and flows.requires_grad and torch.is_grad_enabled():
        return _GatherAtFlowGrad.apply(flows, frame1, frame2, pix, pair, tau, rev, blend)
    out = torch.empty((1 if blend is None else len(blend), n, c), device=frame1.device, dtype=torch.float32)
    return _gather_at_call(_lib.lib().sininn_flow_gather_at, frame1, frame2, flows.detach().contiguous(), pix, pair, tau, rev, blend,
                           (), out)


def bilinear_gather_at(img, pair, qx, qy):
    """sample(I[pair], q) with torch ops at a list: img (B, C, H, W), pair (N,) long inside [0, B), qx, qy (N,) -> (W (N, C), n (N,)).
    `bilinear_gather`'s rule and order of summation."""
    b, c, h, w = img.shape
    flat = img.reshape(b, c, h * w)
    return _tap_walk(qx, qy, h, w, lambda weight, at: weight[:, None] * flat[pair, :, at])


def gather_at_from(frame1, frame2, flows, pix, pair, tau, rev, blend, sample=bilinear_gather_at, eps=GATHER_EPS):
    """The definition of `gather_at`, operation by operation, in the dtype and on the device of the frames.  `sample` and `eps` are
    the places a test swaps in something else."""
    dt, dev = frame1.dtype, frame1.device
    b = frame1.shape[0]
    flows, pix, tau = flows.to(device=dev, dtype=dt), pix.to(device=dev, dtype=dt), tau.to(device=dev, dtype=dt)
    pair = pair.to(dev).long()
    inside = (pair >= 0) & (pair < b)
    at = pair.clamp(0, b - 1)
    py, px = pix[:, 0], pix[:, 1]
    g1 = flows[0, 0:2]
    if flows.shape[0] == 2 and rev is not None:
        back = rev.to(dev).bool()
        g0, c0 = torch.where(back, g1, flows[1, 2:4]), torch.where(back, -tau, tau)
    elif flows.shape[0] == 2:
        g0, c0 = flows[1, 2:4], tau
    else:
        g0, c0 = g1, -tau
    c1 = 1 - tau
    (w0, n0), (w1, n1) = sample(frame1, at, px + c0 * g0[0], py + c0 * g0[1]), sample(frame2, at, px + c1 * g1[0], py + c1 * g1[1])
    h0, h1 = sample(frame1, at, px, py)[0], sample(frame2, at, px, py)[0]
    rows = []
    for a1 in ([tau] if blend is None else [torch.full_like(tau, v) for v in blend]):
        value = _blend(1 - a1, a1, w0, w1, n0, n1, h0, h1, eps, 1)
        rows.append(torch.where(inside[:, None], value, torch.zeros_like(value)))
    return torch.stack(rows)


def gather_at_composed(frame1, frame2, flows, pix, pair, tau, rev=None, *, blend=None, flow_grad=False):
    """`gather_at` from torch ops, on the device and in the dtype of the frames (CPU or GPU, fp32 or fp64; the other float inputs are
    converted to it): the baseline and the reference.  In fp32 it rounds where the fused operator rounds.  `flow_grad=True`: where
    `flows` requires grad the result carries autograd's gradient to it."""
    _, _, _, _, _, _, blend = _gather_at_inputs('gather_at_composed', frame1, frame2, flows, pix, pair, tau, rev, blend, flow_grad)
    assert frame1.dtype in (torch.float32, torch.float64) and frame2.dtype == frame1.dtype
    args = (frame1.detach(), frame2.detach(), flows, pix.detach(), pair, tau.detach(), rev, blend)
    if flow_grad and flows.requires_grad and torch.is_grad_enabled():
        return gather_at_from(*args)
    with torch.no_grad():
        return gather_at_from(*args)


# ---- frame quality ----

Quality = collections.namedtuple('Quality', 'psnr ssim mse map')
WINDOW, SIGMA = 11, 1.5
SSIM_C1, SSIM_C2 = 0.01 ** 2, 0.03 ** 2


def gaussian_window(size=WINDOW, sigma=SIGMA):
    """the normalised 1-D window as Python floats (double): g_i = exp(-(i - size // 2)^2 / (2 sigma^2)) / sum"""
    g = [math.exp(-(i - size // 2) ** 2 / (2 * sigma * sigma)) for i in range(size)]
    total = math.fsum(g)
    return [v / total for v in g]


_WINDOW32 = (C.c_float * WINDOW)(*gaussian_window())


def quality_workspace_floats(b, c, h, w):
    return int(_lib.lib().sininn_frame_quality_workspace_floats(b, c, h, w))


def _quality_inputs(who, pred, target):
    _refuse_grad(who, (pred, target))
    assert pred.shape == target.shape, f'flowsynth.{who}: pred and target differ in shape'
    assert pred.dim() in (4, 5), f'flowsynth.{who}: frames are (B, C, H, W) or (B, K, C, H, W)'
    lead = tuple(pred.shape[:-3])
    c, h, w = pred.shape[-3:]
    if c not in (1, 3):
        raise ValueError(f'flowsynth.{who}: frames have 1 or 3 channels (got {c})')
    if h < WINDOW or w < WINDOW:
        raise ValueError(f'flowsynth.{who}: frames of {h} x {w} are smaller than the {WINDOW} x {WINDOW} window')
    return lead, c, h, w


def quality(pred, target, *, quantize=False, ssim_map=False, workspace=None):
    """PSNR, mean SSIM and MSE of `pred` against `target`, per frame: a `Quality(psnr, ssim, mse, map)` of fp32 device tensors shaped
    like the leading dimensions, (B,) for (B, C, H, W) frames and (B, K) for (B, K, C, H, W); `map` is None, or with `ssim_map=True`
    the per-window SSIM, (..., C, H - 10, W - 10).  `quantize=True`: on the bytes of both frames (see the module text).  `workspace`:
    an fp32 device buffer of at least `quality_workspace_floats(B, C, H, W)` values for the flattened batch (allocated here otherwise;
    needs no initialisation).  Two launches, no atomics, nothing read back: equal inputs give equal bits.  No gradient."""
    lead, c, h, w = _quality_inputs('quality', pred, target)
    pred = _gpu32(pred).reshape(-1, c, h, w).contiguous()
    target = _gpu32(target).reshape(-1, c, h, w).contiguous()
    b, dev = pred.shape[0], pred.device
    need = quality_workspace_floats(b, c, h, w)
    if workspace is None:
        workspace = torch.empty(max(need, 2), device=dev, dtype=torch.float32)
    assert workspace.is_cuda and workspace.dtype == torch.float32 and workspace.is_contiguous(), 'workspace: contiguous fp32 on the device'
    sqerr = torch.empty(max(b, 1), device=dev, dtype=torch.float64)
    out = torch.empty((3, b), device=dev, dtype=torch.float32)
    smap = torch.empty((b, c, h - WINDOW + 1, w - WINDOW + 1), device=dev, dtype=torch.float32) if ssim_map else None
    check(_lib.lib().sininn_frame_quality(ptr(pred), ptr(target), b, c, h, w, int(bool(quantize)), _WINDOW32, ptr(workspace),
                                          workspace.numel(), C.c_void_p(sqerr.data_ptr()), ptr(out), ptr(smap), _stream()))
    if smap is not None:
        smap = smap.reshape(*lead, *smap.shape[1:])
    return Quality(out[1].reshape(lead), out[2].reshape(lead), out[0].reshape(lead), smap)


def to_bytes(x):
    """`synthesize`'s u8 rule as a float tensor of byte values, in the dtype of x: clamp(round-half-even(255 x), 0, 255)"""
    return (x * 255).round().clamp(0, 255)


def quality_composed(pred, target, *, quantize=False, ssim_map=False):
    """`quality` from torch ops, in the dtype and on the device of the inputs (CPU or GPU, fp32 or fp64): per moment two `conv2d` with
    the 1-D Gaussian, along x then along y.  With fp64 inputs it is the reference; in fp32 it rounds where the fused operator rounds,
    except inside the two filters, whose order of accumulation is the library's.  The sums over a frame are carried in float64."""
    lead, c, h, w = _quality_inputs('quality_composed', pred, target)
    with torch.no_grad():
        p = pred.detach().reshape(-1, 1, h, w)
        t = target.detach().reshape(-1, 1, h, w)
        assert p.dtype == t.dtype and p.dtype in (torch.float32, torch.float64), 'quality_composed: fp32 or fp64 frames of one dtype'
        n = c * h * w
        if quantize:
            bp, bt = to_bytes(p), to_bytes(t)
            sqerr = ((bp - bt) ** 2).to(torch.float64).reshape(-1, n).sum(1)        # integers: exact
            mse = sqerr / (65025.0 * n)
            p, t = bp / 255, bt / 255
        else:
            d = p - t
            sqerr = (d * d).to(torch.float64).reshape(-1, n).sum(1)
            mse = sqerr / n
        psnr = torch.where(mse == 0, torch.full_like(mse, math.inf), 10 * torch.log10(1 / mse))
        g = torch.tensor(gaussian_window(), dtype=p.dtype, device=p.device)
        gx, gy = g.view(1, 1, 1, WINDOW), g.view(1, 1, WINDOW, 1)

        def filt(x):
            return torch.nn.functional.conv2d(torch.nn.functional.conv2d(x, gx), gy)

        mp, mt = filt(p), filt(t)
        mpp, mtt, mpt = mp * mp, mt * mt, mp * mt
        s_p, s_t, s_pt = filt(p * p) - mpp, filt(t * t) - mtt, filt(p * t) - mpt
        smap = ((2 * mpt + SSIM_C1) * (2 * s_pt + SSIM_C2)) / ((mpp + mtt + SSIM_C1) * (s_p + s_t + SSIM_C2))
        smap = smap.reshape(*lead, c, h - WINDOW + 1, w - WINDOW + 1)
        ssim = smap.to(torch.float64).flatten(-3).mean(-1)
        dt = pred.dtype
        return Quality(psnr.to(dt).reshape(lead), ssim.to(dt).reshape(lead), mse.to(dt).reshape(lead), smap if ssim_map else None)
