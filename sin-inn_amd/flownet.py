"""The flow-field network of the flow trainer: a coordinate MLP evaluated at every pixel of every frame, forward and
backward in libsininn.so (csrc/flownet.hip).

    ModelParams / RbfModel / FFModel / UFFModel / model_dict   video-interpolation/model.py:11-28, 490-505, 418-433, 454-469, 681
    ProgressiveModel / PRBFModel / PFFModel / PUFFModel        video-interpolation/model.py:526-598, 621-625 (progressive_model_dict)
    RotatedFourierFeatures / RFFModel / PRFFModel              video-interpolation/model.py:263-307, 436-451, 586-590 (learnable_model_dict)
    UniformRadialBasisGridEncoding / RbfgModel / PRBFGModel    video-interpolation/model.py:369-415, 508-523, 614-618 (grid_model_dict)
    PositionalEncoding / PEModel / PPEModel                    video-interpolation/model.py:321-340, 472-487, 607-611 (positional_model_dict)
    SineLayer / SirenModel                                     video-interpolation/model.py:123-146, 149-171 (siren_model_dict)
    PieceWiseEncoding / MPFFModel                              video-interpolation/model.py:628-678, 600-604 (piecewise_model_dict)
    flow_fields                                                FlowTrainer.forward, video-interpolation/trainer.py:37-45
    flow_at / net(poses)                                       net(poses) of trainer.py:43-44, pair_flow.py:58-59

The modules have the reference's constructor signatures, its `state_dict` keys (`encode.centres`, `encode.sigma` /
`encode.frequencies` / `encode.offsets`, `encode.sigma` / `encode.freqs`, `model.model.{0,2,4,6}.{weight,bias}`) and its order of RNG draws at construction (encoding buffers
first, then the four nn.Linear layers), so one `torch.manual_seed` gives the reference's numbers and a reference checkpoint
loads.  One table describes them: `ENCODINGS` holds each encoding's constructor call once, a model class names its row and is plain or
progressive, and `all_model_dict` maps the twelve network names to the classes; the reference's five dicts are views of it.  The
encodings of `model_dict` / `progressive_model_dict` / `grid_model_dict` are buffers: no gradient flows below layer 1.  The kernels are
built for the ModelParams defaults; any other size raises with the library's own list of the sizes it supports, there is no second
implementation behind this module.  On a grid the N x 3 pose list never exists; on a pose list (`flow_at`, below) it is the caller's
tensor, read in place; the N x 512 encoding never exists in either.

The progressive models feed `cat((t, y, x), encode(x)) * mask` to layer 1 (515 features, first weight [256][515]); the mask is
a global vector of 515 values that a controller of `sin_inn_amd.progressive` opens block by block (main.py:136-143).
`flow_fields` takes a bare progressive model (all-ones mask: the reference applies none) or a controller, and an
`override_mask` that beats the controller's own (progressive_controller.py:45-53).  The controller's mask comes with the
number of leading features it has opened so far, and the kernels skip the rest of layer 1; an `override_mask` given as a device
tensor is not inspected on the host and runs over all 515 features.  Both give bitwise the same result.

`RFF` / `PRFF` train the encoding itself: `encode.frequencies` is an nn.Parameter [3][256] and the network uses
`F_eff = normalize(frequencies, dim=0) * magnitudes` (`magnitudes` a buffer).  `flow_fields` computes F_eff with torch ops under
autograd on every call (768 values) and hands it to the kernels as the frequency matrix, so the forward pass is the Fourier one;
the backward pass (`sininn_flownet_backward` in its ENCGRAD mode) carries the gradient through layer 1 onto F_eff, all in fp32 with a fixed
summation order, and torch's `normalize` backward takes it to `encode.frequencies.grad`.  With `frequencies.requires_grad` false,
or grad mode off, the plain backward / inference path runs and nothing extra is computed.

`RBFG` / `PRBFG` use a periodic grid of Gaussian bumps: 256 frequencies j with buffers `encode.offsets` [256][3] and `encode.sigma`
[256] (`linspace(0, 12 sqrt(3), 256)` plus half a step), period p = 2 / sigma_j.  Feature 2 j is
`2 exp(-sigma_j^2 |((x + offsets_j) mod p) 2 - p|^2) - 1`, feature 2 j + 1 the same half a period further
(`+ 1 / sigma_j`).  Both are buffers, the kernels evaluate them as an encoding of their own (`RBFG = 3`) and the rest (masks, `k_active`, the
backward pass) is the path of `RBF` / `PRBF`.

`PE` / `PPE` use the axis-aligned positional encoding of NeRF: the buffer `encode.freqs` = 2^i pi (i = 0 .. 3, fp32), feature
`6 f + d` is `cos(freqs[f] x_d)` and feature `6 f + 3 + d` is `sin(freqs[f] x_d)`: 24 features, the cosines of a frequency before
its sines.  Layer 1 is [256][24] (PPE: [256][27], mask of 27 values, blocks of 6 that cut through a frequency).  The reference's
`PositionalEncoding.forward` reshapes through `.view(-1, 21)` (model.py:332), which raises unless the number of points is a
multiple of 7 and is the formula above where it runs; the kernels evaluate the formula for every N.  In the kernels it is the one
encoding with a narrow layer 1 (two 16-feature K steps instead of 32, a 32-column weight-gradient tile).

`MPFF` (`MPFFModel`, progressive only) uses the piecewise-linear encoding: the buffer `encode.frequencies` [3][256] (non-negative, columns
of ascending magnitude), u = (x + 1) @ frequencies, feature 2 f = tri(u_f), feature 2 f + 1 = tri(u_f + 1) with
`tri(w) = 2 r + 1 if r < 0 else 1 - 2 r`, `r = fmod(w, 2) - 1` and torch.fmod's truncation: a triangle wave of period 2 for w >= 0, and for
w < 0 (points outside [-1, 1]^3) the reference's own values in (-5, -1], reproduced as they are.  An encoding of its own in the kernels
(`PIECEWISE = 5`), the rest is the path of `PFF`: global masks and `k_active`, the spatial controller, pose lists, and a coordinate gradient
that is piecewise constant (-+2 F[d][f], the sign of the branch the forward pass took).  The reference's `model_dict` does not hold it and
neither does `all_model_dict`: it is registered in `piecewise_model_dict`, beside it, and the command line stays closed.

`siren` (`SirenModel`) has no encoding: four `SineLayer`s, `sin(30 (W h + b))`, the first on the three raw coordinates, and a plain
last nn.Linear (`state_dict` keys `model.{0..3}.linear.{weight,bias}`, `model.4.{weight,bias}`; every nn.Linear draws its own init first,
then `weight.uniform_`).  It runs in kernels of its own (csrc/siren.hip, `siren_forward` / `siren_backward`) behind the same
`flow_fields`; the sine is the accurate full-range fp32 function and omega is passed on every call.  It is registered in
`siren_model_dict`, beside `all_model_dict`, not in it.

Spatially adaptive progression (`sin_inn_amd.progressive.StashedSpatialController`, the reference's `--spatially-adaptive`): every
point has its own 515 mask values, interpolated trilinearly from the controller's blurred grid [res^3][515] on the device.  The
per-point mask never exists in memory either: the kernels sample the grid while they generate the operand of layer 1
(`flownet_forward_spatial` / `flownet_backward_spatial`, the SPATIAL mode), W1 is read in place and there is no pack step.
`flow_fields` takes that controller (`k_active` = its `next_block`), or a raw grid as a 2-D `override_mask`; `flownet_sample_mask`
returns the interpolated mask itself (the reference's `get_mask=` keyword).  The networks with the table's `spatial` (flowcaps.py).

One call path serves every mode.  The library has five run entry points, `sininn_{flownet,siren}_{forward,backward}` and
`sininn_flownet_sample_mask`; each takes the network descriptor and, beside it, a call descriptor (`_lib.FlowNetCall`) whose mode bits say
what the call is: AT_POINTS (a pose list, not the descriptor's grid), SPATIAL (a per-point mask), ENCGRAD / POSEGRAD (the backward call also
returns the frequency / the coordinate gradient), and the number of coordinates.  `Mask` is the mask of a call: the device tensor,
`k_active` and, for a grid, `res` and `centre_scale`; `.spatial` is the one way to ask which it is, and `_resolve_mask`, the controllers'
`device_mask` / `device_grid`, `_FlowFields` and `flow_fields` pass it around.  A network descriptor is built by `_args` / `_siren_args`, which
share the points (a grid or a pose list) and the layers (`_points_and_layers`); `_call` builds the call descriptor from it, one clause per
bit; `_forward` allocates `flows` / `saved` and calls, `_backward` checks `dflows`, allocates the workspace and the gradients, calls, and returns
the extra gradients the mode asked for.  The public forward / backward functions name their two builders and nothing else; `_FlowFields` and
`_FlowAt` are the two autograd functions over one body (`_fields_forward` / `_fields_backward`), `_functions` picks the pair of functions and
their keyword arguments for them (`_SirenFields.apply` is the SIREN call of `_FlowFields` under the earlier name).

Arbitrary points: `flow_at(net, poses, scale)` and, through it, `net(poses)` and `controller(poses, override_mask=, get_mask=)`
evaluate the same kernels at a caller's pose list (..., 3) -> (..., 4) (the AT_POINTS mode): the kernels
read point p's coordinates from row p of the list where the grid mode reads the three axis vectors, and nothing else differs, so the
flows and gradients of a list that spells out a grid are bitwise those of the grid call.  The kernels write the planar (4, N) layout
(`planar=True` returns it); the transpose to the reference's (N, 4) is a torch op.  Differentiable with respect to the parameters
(`_FlowAt`, next to `_FlowFields`), learnable frequencies included, and, with `pose_grad=True`, with respect to the coordinates: the
backward pass then runs in the POSEGRAD mode, which contracts dh1 W1 with the
analytic derivative of the encoding over the features of each point (csrc/flownet.hip, flownet_posegrad_kernel).

Per-point masks at pose lists: `controller(poses)` of a `StashedSpatialController` is the reference's own way to evaluate one
(progressive_controller.py:670-680), and `flow_at` takes that controller, or any controller with a grid (res^3, 515) on the device as a 2-D
`override_mask`.  The calls are `flownet_forward_spatial_points` / `flownet_backward_spatial_points` / `flownet_sample_mask_points`
(AT_POINTS | SPATIAL): the spatial kernels at a pose list, bitwise the spatial grid call where the list spells out a grid;
`pose_grad=True` runs the SPATIAL form of flownet_posegrad_kernel.  The mask is a constant of the point there, as in the reference, which
interpolates it under no_grad: the pose gradient has no d mask / d pose term.  A bare progressive model with a grid is still refused at a
pose list: the interpolation is a controller's.

Two coordinates (`ModelParams(domain_dim=2)`, the network of video-interpolation/pair_flow.py:39-42): the networks with the table's `pair`
are built on (y, x) with the reference's layouts (`encode.centres` [512][2], `encode.frequencies`
[2][256], `encode.offsets` [256][2], a progressive first weight [256][514] = the columns of cat((y, x), enc)) and run in the DIM = 2
instantiations of the kernels (`domain_dim = 2` in the call descriptor, beside the unchanged network descriptor).
`flow_fields(net_or_controller, None, h, w, scale)` is one frame pair, poses linspace(-1, 1, h) x linspace(-1, 1, w) (pair_flow.py:55-59),
flows (1, 4, h, w): `times` must be None.  `flow_at`, `net(poses)` and `controller(poses, ..)` take (..., 2) -> (..., 4).  The global mask has
514 values in blocks of 4, `override_mask`, `get_mask` and `k_active` work as at three coordinates.  Refused there, each with a ValueError
that names the dimension and the mode (`_refuse_pair_modes`): the other networks, the modes of `flowcaps.PAIR_MODES`, `times` for such a
network, and poses of the other dimension either way.

Which network serves which call (two coordinates, per-point masks, the frequency, pose and Jacobian gradients, the command line) is the table
of `sin_inn_amd/flowcaps.py`: every refusal of this module that is about the network reads it, and a network or a mode is
added there.  Out of scope beside it: a plain (non-progressive) piecewise network, the `alpha=` keyword of
ProgressiveModel.apply_control, `FixedSpatialController`, `AdaptiveController`.  Sintel / .flo IO and the trainer are `sin_inn_amd.flowdata` and
`sin_inn_amd.flowtrainer`.  The optimiser: these modules expose ordinary nn.Parameters;
`sin_inn_amd.FusedLAMB` is the reference's apex FusedLAMB (trainer.py:134-135) restated, `sin_inn_amd.FusedAdam` drives them as well.
"""
import ctypes as C
import math
from typing import NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as nnf

from . import _lib, flowcaps
from .flowcaps import FOURIER, PE, PIECEWISE, RBF, RBFG
from .ops import _stream, ptr

check = _lib.check
EPSILON = 1e-4


class ModelParams:
    """model.py:11-28."""

    def fill_args(self, **kwargs):
        for key, item in kwargs.items():
            if hasattr(self, key):
                setattr(self, key, item)

    def __init__(self, **kwargs):
        self.domain_dim = 3
        self.num_frequencies = 256
        self.std = 25
        self.power = 20
        self.num_layers = 3
        self.hidden_dim = 256
        self.output_channels = 4
        self.num_frequencies_pe = 4
        self.std_rbf = 12
        self.fill_args(**kwargs)


class MLP(nn.Module):
    """model.py:31-43: Linear / ReLU chain under `.model` (state_dict keys model.{0,2,4,..})."""

    def __init__(self, layers):
        super().__init__()
        seq = []
        for i in range(len(layers) - 1):
            seq.append(nn.Linear(layers[i], layers[i + 1]))
            if i < len(layers) - 2:
                seq.append(nn.ReLU(True))
        self.model = nn.Sequential(*seq)


class RadialBasisEncoding(nn.Module):
    """model.py:343-366 (buffers only; evaluated inside the kernels)."""
    kind = RBF

    def __init__(self, domain_dim, num_frequencies, std):
        super().__init__()
        self.domain_dim = domain_dim
        self.num_frequencies = num_frequencies * 2
        centres = torch.rand(self.num_frequencies, domain_dim) * 2 - 1
        sigma = torch.randn(self.num_frequencies).abs() * std + 1
        self.register_buffer('centres', centres)
        self.register_buffer('sigma', sigma.sort()[0])

    @property
    def output_channels(self):
        return self.num_frequencies

    def kernel_buffers(self):
        return self.centres, self.sigma


class _FourierFeatures(nn.Module):
    """model.py:224-249."""
    kind = FOURIER

    def __init__(self, domain_dim, num_frequencies, std):
        super().__init__()
        self.domain_dim = domain_dim
        self.num_frequencies = num_frequencies
        magnitude = self.init_magnitude(std)
        magnitude = magnitude[magnitude.abs().argsort(0)]
        frequencies = torch.randn(domain_dim, num_frequencies)
        self.register_buffer('frequencies', nnf.normalize(frequencies, p=2, dim=0) * magnitude[None, :])

    @property
    def output_channels(self):
        return self.num_frequencies * 2

    def kernel_buffers(self):
        return self.frequencies, None


class GaussianRandomFourierFeatures(_FourierFeatures):
    """model.py:252-260."""

    def init_magnitude(self, std):
        return torch.randn(self.num_frequencies) * std


class UniformFourierFeatures(_FourierFeatures):
    """model.py:309-318."""

    def init_magnitude(self, std):
        std = std / math.sqrt(3)
        return torch.linspace(-std, std, self.num_frequencies) + EPSILON


class RotatedFourierFeatures(nn.Module):
    """model.py:263-297: unit-norm directions are trained, the magnitudes are a buffer.  `init_magnitudes` is drawn first, then the
    directions; the parameter is registered after the buffer but leads the state dict (parameters come before buffers)."""
    kind = FOURIER

    def __init__(self, domain_dim, num_frequencies, std):
        super().__init__()
        self.domain_dim = domain_dim
        self.num_frequencies = num_frequencies
        magnitudes = self.init_magnitudes(std)
        frequencies = nn.Parameter(nnf.normalize(torch.randn(domain_dim, num_frequencies), p=2, dim=0))
        self.register_buffer('magnitudes', magnitudes)
        self.register_parameter('frequencies', frequencies)

    @property
    def output_channels(self):
        return self.num_frequencies * 2

    def effective_frequencies(self):
        """F_eff [3][256] (model.py:274), differentiable with respect to `frequencies`"""
        return nnf.normalize(self.frequencies, p=2, dim=0) * self.magnitudes[None, :]

    def kernel_buffers(self):
        return self.effective_frequencies().detach().contiguous(), None


class GaussianRotatedFourierFeatures(RotatedFourierFeatures):
    """model.py:299-307: the sorted magnitudes; the reference then draws a (domain_dim, num_frequencies) normal sample that it does
    not use, which moves the generator, so it is drawn here too."""

    def init_magnitudes(self, std):
        magnitude = torch.randn(self.num_frequencies) * std
        magnitude = magnitude[magnitude.abs().argsort(0)]
        torch.randn(self.domain_dim, self.num_frequencies)
        return magnitude


class UniformRadialBasisGridEncoding(nn.Module):
    """model.py:369-415 (buffers only; evaluated inside the kernels).  The one RNG draw is the `rand` of the offsets; `sigma` is
    ascending as built, the reference's sort leaves it as it is."""
    kind = RBFG

    def __init__(self, domain_dim, num_frequencies, std):
        super().__init__()
        self.domain_dim = domain_dim
        self.num_frequencies = num_frequencies
        sigma = torch.linspace(0, std * math.sqrt(3), num_frequencies)
        sigma = sigma + sigma[1] / 2
        offsets = (torch.rand(num_frequencies, domain_dim) * 2 - 1) % (2 / sigma[:, None])
        self.register_buffer('offsets', offsets)
        self.register_buffer('sigma', sigma.sort()[0])

    @property
    def output_channels(self):
        return 2 * self.num_frequencies

    def kernel_buffers(self):
        return self.offsets, self.sigma


class PositionalEncoding(nn.Module):
    """model.py:321-340 (one buffer, no RNG draw; evaluated inside the kernels).  Feature 6 f + d = cos(freqs[f] x_d), feature
    6 f + 3 + d = sin(freqs[f] x_d).  The reference's forward runs only where the number of points is a multiple of 7 (its
    `.view(-1, 21)`), and is this formula there; the kernels evaluate it for every N."""
    kind = PE

    def __init__(self, domain_dim, num_frequencies):
        super().__init__()
        self.domain_dim = domain_dim
        self.num_frequencies = num_frequencies
        self.register_buffer('freqs', torch.tensor([2. ** i * math.pi for i in range(num_frequencies)]))

    @property
    def output_channels(self):
        return self.num_frequencies * self.domain_dim * 2

    def kernel_buffers(self):
        return self.freqs, None


class PieceWiseEncoding(nn.Module):
    """model.py:628-657 (one buffer; evaluated inside the kernels): u = (x + 1) @ frequencies, features tri(u), tri(u + 1) interleaved,
    tri(w) = 2 r + 1 if r < 0 else 1 - 2 r with r = fmod(w, 2) - 1 (torch.fmod: the sign of w)."""
    kind = PIECEWISE

    def __init__(self, domain_dim, num_frequencies, std):
        super().__init__()
        self.domain_dim = domain_dim
        self.num_frequencies = num_frequencies
        self.register_buffer('frequencies', self.init_frequencies(std))

    @property
    def output_channels(self):
        return 2 * self.num_frequencies

    def kernel_buffers(self):
        return self.frequencies, None


class GaussianRandomPieceWiseEncoding(PieceWiseEncoding):
    """model.py:660-667: |N(0, std / 2 pi)| per entry, the columns sorted by their norm."""

    def init_frequencies(self, std):
        frequencies = torch.randn(self.domain_dim, self.num_frequencies) * std / (2 * math.pi)
        frequencies = frequencies.abs()
        order = frequencies.norm(2, 0).argsort()
        return frequencies[:, order]


class UniformPieceWiseEncoding(PieceWiseEncoding):
    """model.py:670-678: magnitudes linspace(0, std sqrt(12) / 2 pi) plus half a step, along the absolute values of one normal draw
    (domain_dim, num_frequencies), normalised per column.  The bound is a float64 scalar, as the reference's numpy expression is."""

    def init_frequencies(self, std):
        b = std * math.sqrt(12) / (2 * math.pi)
        magnitude = torch.linspace(0, b, self.num_frequencies)
        magnitude = magnitude + magnitude[1] / 2
        frequencies = torch.randn(self.domain_dim, self.num_frequencies).abs()
        return nnf.normalize(frequencies, p=2, dim=0) * magnitude[None, :]


# encoding name -> its one constructor call; the plain and the progressive model of an encoding share it
ENCODINGS = {
    'RBF': lambda opt: RadialBasisEncoding(opt.domain_dim, opt.num_frequencies, opt.std_rbf),
    'FFN': lambda opt: GaussianRandomFourierFeatures(opt.domain_dim, opt.num_frequencies, opt.std),
    'UFF': lambda opt: UniformFourierFeatures(opt.domain_dim, opt.num_frequencies, opt.std),
    'RFF': lambda opt: GaussianRotatedFourierFeatures(opt.domain_dim, opt.num_frequencies, opt.std),
    'RBFG': lambda opt: UniformRadialBasisGridEncoding(opt.domain_dim, opt.num_frequencies, opt.std_rbf),
    'PE': lambda opt: PositionalEncoding(opt.domain_dim, opt.num_frequencies_pe),
    'MPFF': lambda opt: UniformPieceWiseEncoding(opt.domain_dim, opt.num_frequencies, opt.std),
    'GMPFF': lambda opt: GaussianRandomPieceWiseEncoding(opt.domain_dim, opt.num_frequencies, opt.std),   # no reference network names it
}


class _EncodedMlpModel(nn.Module):
    """model.py:54-103, the part the flow trainer uses: `encode` is drawn first, then the MLP on `encoding_dim` inputs.  A model
    class names its row of ENCODINGS."""
    encoding = None
    is_progressive = False

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.encode = ENCODINGS[self.encoding](opt)
        self.model = MLP([self.encoding_dim] + opt.num_layers * [opt.hidden_dim] + [opt.output_channels])
        self._axes = {}
        self._ones = {}

    @property
    def encoding_dim(self):
        return self.encode.output_channels

    @property
    def domain_dim(self):
        return self.opt.domain_dim

    def update_progress(self):
        return

    def stash_iteration(self, *args):
        return

    def linears(self):
        return [m for m in self.model.model if isinstance(m, nn.Linear)]

    def forward(self, x, *args, **kwargs):
        """net(poses), model.py:97-103: (..., 3) -> (..., 4) in the fused kernels (`flow_at`); `jacobian=` is flow_at's"""
        return flow_at(self, x, 1.0, override_mask=kwargs.get('override_mask'), pose_grad=kwargs.get('pose_grad', False),
                       jacobian=kwargs.get('jacobian'))


class ProgressiveModel(_EncodedMlpModel):
    """model.py:526-576: layer 1 reads cat((x, encode(x))) times a mask: the MLP has 515 inputs (PPE: 27)."""
    is_progressive = True

    @property
    def encoding_dim(self):
        return self.encode.output_channels + self.domain_dim

    def ones_mask(self, device):
        """the mask of a network evaluated without a controller, cached per device"""
        if device not in self._ones:
            self._ones[device] = torch.ones(self.encoding_dim, device=device)
        return self._ones[device]


def _model(name, base, encoding, doc):
    return type(name, (base,), {'encoding': encoding, '__doc__': doc, '__module__': __name__})


# the registry: network name -> model class = (row of ENCODINGS, progressive?)
RbfModel = _model('RbfModel', _EncodedMlpModel, 'RBF', 'model.py:490-505.')
FFModel = _model('FFModel', _EncodedMlpModel, 'FFN', 'model.py:418-433.')
UFFModel = _model('UFFModel', _EncodedMlpModel, 'UFF', 'model.py:454-469.')
PRBFModel = _model('PRBFModel', ProgressiveModel, 'RBF', 'model.py:621-625.')
PFFModel = _model('PFFModel', ProgressiveModel, 'FFN', 'model.py:579-583.')
PUFFModel = _model('PUFFModel', ProgressiveModel, 'UFF', 'model.py:593-597.')
RFFModel = _model('RFFModel', _EncodedMlpModel, 'RFF', 'model.py:436-451.')
PRFFModel = _model('PRFFModel', ProgressiveModel, 'RFF', 'model.py:586-590.')
RbfgModel = _model('RbfgModel', _EncodedMlpModel, 'RBFG', 'model.py:508-523.')
PRBFGModel = _model('PRBFGModel', ProgressiveModel, 'RBFG', 'model.py:614-618.')
PEModel = _model('PEModel', _EncodedMlpModel, 'PE', 'model.py:472-487.')
PPEModel = _model('PPEModel', ProgressiveModel, 'PE', 'model.py:607-611.')
all_model_dict = {'RBF': RbfModel, 'FFN': FFModel, 'UFF': UFFModel, 'PRBF': PRBFModel, 'PFF': PFFModel, 'PUFF': PUFFModel,
                  'RFF': RFFModel, 'PRFF': PRFFModel, 'RBFG': RbfgModel, 'PRBFG': PRBFGModel, 'PE': PEModel, 'PPE': PPEModel}


def _view(*names):
    return {name: all_model_dict[name] for name in names}


# the reference's five dicts, as views of the registry
model_dict = _view('RBF', 'FFN', 'UFF')
progressive_model_dict = _view('PRBF', 'PFF', 'PUFF')
learnable_model_dict = _view('RFF', 'PRFF')                       # the encoding is trained; PRFF is progressive as well
grid_model_dict = _view('RBFG', 'PRBFG')                          # the radial-basis grid; PRBFG is progressive
positional_model_dict = _view('PE', 'PPE')                        # 24 features; PPE is progressive


class SineLayer(nn.Module):
    """model.py:123-146: sin(omega_0 * linear(x)); nn.Linear's own init draws first, then `weight.uniform_`.  Evaluated inside the
    kernels."""

    def __init__(self, in_features, out_features, bias=True, is_first=False, omega_0=30):
        super().__init__()
        self.omega_0 = omega_0
        self.is_first = is_first
        self.in_features = in_features
        self.linear = nn.Linear(in_features, out_features, bias=bias)
        self.init_weights()

    def init_weights(self):
        with torch.no_grad():
            if self.is_first:
                self.linear.weight.uniform_(-1 / self.in_features, 1 / self.in_features)
            else:
                bound = math.sqrt(6 / self.in_features) / self.omega_0
                self.linear.weight.uniform_(-bound, bound)


class SirenModel(nn.Module):
    """model.py:149-171: SineLayer(3, 256, first), 3 x SineLayer(256, 256), nn.Linear(256, 4) with `weight.uniform_` after its own
    init; `model` is the nn.Sequential of the five."""
    is_progressive = False

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        layers = [SineLayer(opt.domain_dim, opt.hidden_dim, is_first=True, omega_0=30)]
        for _ in range(opt.num_layers):
            layers.append(SineLayer(opt.hidden_dim, opt.hidden_dim, is_first=False, omega_0=30))
        final_linear = nn.Linear(opt.hidden_dim, opt.output_channels)
        with torch.no_grad():
            bound = math.sqrt(6 / opt.hidden_dim) / 30
            final_linear.weight.uniform_(-bound, bound)
        layers.append(final_linear)
        self.model = nn.Sequential(*layers)
        self._axes = {}

    @property
    def encoding_dim(self):
        return self.opt.domain_dim

    @property
    def domain_dim(self):
        return self.opt.domain_dim

    @property
    def omega(self):
        """omega_0 of the sine layers: one value, the kernels take it as an argument"""
        omegas = {m.omega_0 for m in self.model if isinstance(m, SineLayer)}
        if len(omegas) != 1:
            raise ValueError(f'siren kernels take one omega for every sine layer; got {sorted(omegas)}')
        return float(omegas.pop())

    def update_progress(self):
        return

    def stash_iteration(self, *args):
        return

    def linears(self):
        return [m.linear if isinstance(m, SineLayer) else m for m in self.model]

    def forward(self, x, *args, **kwargs):
        """net(poses), model.py:167-171: (..., 3) -> (..., 4) in the fused kernels (`flow_at`); `jacobian=` is flow_at's (and refused)"""
        return flow_at(self, x, 1.0, override_mask=kwargs.get('override_mask'), pose_grad=kwargs.get('pose_grad', False),
                       jacobian=kwargs.get('jacobian'))


# the piecewise-linear progressive network (model.py:600-604): beside all_model_dict, like siren; the reference's model_dict lacks it too
MPFFModel = _model('MPFFModel', ProgressiveModel, 'MPFF', 'model.py:600-604.')
piecewise_model_dict = {'MPFF': MPFFModel}
siren_model_dict = {'siren': SirenModel}                          # beside all_model_dict: the command line does not open it yet
flow_model_dict = {**all_model_dict, **piecewise_model_dict, **siren_model_dict}          # every network flow_fields evaluates: what the tools offer


def _on_gpu(t, what='tensor'):
    if not t.is_cuda:
        raise NotImplementedError(f'sin-inn_amd flownet runs on the GPU only (got a CPU {what})')


IDENTITY_SCALE = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)


class Mask(NamedTuple):
    """The mask of one call.  `tensor`: None (a plain network), the global mask (enc_dim,) or the grid (res^3, enc_dim), on the device;
    `k_active`: the number of leading features after which it is all zero (None: nothing is skipped); a grid comes with its `res` and
    `centre_scale`, six host floats, centre (t, y, x) then scale (t, y, x)."""
    tensor: Optional[torch.Tensor] = None
    k_active: Optional[int] = None
    res: Optional[int] = None
    centre_scale: Optional[tuple] = None

    @property
    def spatial(self):
        return self.res is not None


# ---- the descriptors: what is particular to a kind of network, then the part they share ----
def _points_and_layers(a, lins, times, ys, xs, scale, dim=3):
    """the grid of points (axes on the GPU, T H W, scale, pointers) and the nn.Linear layers of a descriptor.  `ys is None`: `times`
    is a pose list (N, dim); the descriptor gets the planar shape T = H = 1, W = N that `flows` / `dflows` have then and no axis
    pointers, and `a._poses` is what the call descriptor takes of it (None on a grid).  `dim == 2` on a grid: the axes are (ys, xs), `times`
    is None and T = 1"""
    if ys is None:
        poses = times
        _on_gpu(poses, 'pose list')
        assert poses.dtype == torch.float32 and poses.dim() == 2 and poses.shape[1] == dim, f'a pose list (N, {dim}), fp32'
        poses = poses.contiguous()
        a.T, a.H, a.W, a.scale = 1, 1, poses.shape[0], float(scale)
        a._axes, a._device = (poses,), poses.device
        a._poses = (ptr(poses) if poses.numel() else None, poses.shape[0])
    elif dim == 2:
        if times is not None:
            raise ValueError('domain_dim 2: a network on (y, x) has no times; pass times=None')
        for t in (ys, xs):
            _on_gpu(t)
        ys, xs = ys.contiguous(), xs.contiguous()
        a.T, a.H, a.W, a.scale = 1, ys.numel(), xs.numel(), float(scale)
        a.ys, a.xs = ptr(ys), ptr(xs)
        a._axes, a._device, a._poses = (ys, xs), ys.device, None
    else:
        for t in (times, ys, xs):
            _on_gpu(t)
        times, ys, xs = times.contiguous(), ys.contiguous(), xs.contiguous()
        a.T, a.H, a.W, a.scale = times.numel(), ys.numel(), xs.numel(), float(scale)
        a.times, a.ys, a.xs = ptr(times), ptr(ys), ptr(xs)
        a._axes, a._device, a._poses = (times, ys, xs), times.device, None   # the contiguous copies live as long as the descriptor
    for l, lin in enumerate(lins):
        _on_gpu(lin.weight, 'parameter')
        assert lin.weight.is_contiguous() and lin.bias.is_contiguous()
        a.w[l], a.b[l] = ptr(lin.weight), ptr(lin.bias)
    return a


def _row(net):
    """(model, its row of flowcaps.TABLE) of a model or a controller: found by what the kernels evaluate"""
    from .progressive import ProgressiveEncoderController
    model = net.model if isinstance(net, ProgressiveEncoderController) else net
    enc = getattr(model, 'encode', None)
    return model, flowcaps.BY_ENCODING[getattr(enc, 'kind', None), isinstance(enc, RotatedFourierFeatures)]


def _refuse_pair_modes(net, dim, spatial=False, enc_a=None, pose_grad=False):
    """a network with domain_dim != 3: what the kernels do not do for it, each refusal under the dimension and the mode"""
    if dim != 2:
        raise ValueError(f'domain_dim {dim}: the flownet kernels take 3 coordinates per point (t, y, x) or 2 (y, x)')
    row = _row(net)[1]
    if enc_a is not None and row.kind is not None:       # a frequency matrix of the caller's is the learnable call, whatever the class
        row = flowcaps.TABLE['RFF']
    flowcaps.refuse(row, 'pair', 'domain_dim 2')
    if spatial:
        flowcaps.refuse(flowcaps.PAIR_MODES, 'spatial', 'domain_dim 2')
    if pose_grad:
        flowcaps.refuse(flowcaps.PAIR_MODES, 'pose_grad', 'domain_dim 2')


def _call_dim(net, override_mask=None, pose_grad=False):
    """domain_dim of a model or a controller; other than 3: every refusal of that dimension that a public call can meet, before any
    device is looked at"""
    dim = net.domain_dim
    if dim != 3:
        _refuse_pair_modes(net, dim, override_mask is not None and override_mask.dim() == 2, pose_grad=pose_grad)
    return dim


def _args(net, times, ys, xs, scale, mask=None, k_active=None, enc_a=None, spatial=False):
    lins = net.linears()
    a = _lib.FlowNetArgs()
    a.encoding = net.encode.kind
    a.progressive = int(bool(net.is_progressive))
    a.enc_dim, a.hidden, a.layers, a.out_dim = net.encoding_dim, net.opt.hidden_dim, net.opt.num_layers, net.opt.output_channels
    dim = a._dim = int(net.opt.domain_dim)               # travels beside the descriptor, in the call descriptor
    if dim != 3:
        _refuse_pair_modes(net, dim, spatial, enc_a)
    if not _lib.lib().sininn_flownet_supported_dim(C.byref(a), dim):   # the library's refusal names the sizes it is built for
        raise ValueError(_lib.lib().sininn_last_error().decode())
    if len(lins) != 4:
        raise ValueError(f'flownet kernels take 4 linear layers; got {len(lins)}')
    if spatial:                                          # the grid goes beside the descriptor, its `mask` is ignored
        if not a.progressive:
            raise ValueError('a spatial mask needs a progressive network')
        a.k_active = a.enc_dim if k_active is None else int(k_active)
    elif a.progressive:
        if mask is None:
            raise ValueError('a progressive network is evaluated under a mask (flow_fields supplies all ones for a bare model)')
        _on_gpu(mask, 'mask')
        assert mask.dtype == torch.float32 and mask.is_contiguous() and tuple(mask.shape) == (a.enc_dim,)
        a.mask = ptr(mask)
        a.k_active = a.enc_dim if k_active is None else int(k_active)
    elif mask is not None:
        raise ValueError('a mask needs a progressive network')
    _points_and_layers(a, lins, times, ys, xs, scale, dim)
    if enc_a is None:
        ea, eb = net.encode.kernel_buffers()
    else:                                                # learnable frequencies: F_eff of this call
        _on_gpu(enc_a)
        assert net.encode.kind == FOURIER and enc_a.dtype == torch.float32 and enc_a.is_contiguous() and tuple(enc_a.shape) == (3, 256)
        ea, eb = enc_a, None
    a.enc_a, a.enc_b = ptr(ea), ptr(eb)
    a._keep = (ea, eb)                                   # kernel_buffers() of a learnable encoding is a temporary
    return a


def _siren_args(net, times, ys, xs, scale, omega=None):
    lins = net.linears()
    a = _lib.SirenArgs()
    a.in_dim, a.hidden, a.layers, a.out_dim = net.opt.domain_dim, net.opt.hidden_dim, net.opt.num_layers, net.opt.output_channels
    a.omega = net.omega if omega is None else float(omega)
    if not _lib.lib().sininn_siren_supported(C.byref(a)):        # the library's refusal names the sizes it is built for
        why = _lib.lib().sininn_last_error().decode()
        if net.opt.domain_dim != 3:
            why += f' (domain_dim {net.opt.domain_dim}: the SIREN kernels take three coordinates)'
        raise ValueError(why)
    if len(lins) != 5:
        raise ValueError(f'siren kernels take 5 linear layers; got {len(lins)}')
    a._dim = 3
    return _points_and_layers(a, lins, times, ys, xs, scale)


def _spatial(a, grid, res, centre_scale):
    """(device grid, res, the six host floats) as the call descriptor takes them, checked against the descriptor"""
    _on_gpu(grid, 'mask grid')
    res = int(res)
    assert grid.dtype == torch.float32 and grid.is_contiguous() and tuple(grid.shape) == (res ** 3, a.enc_dim), \
        f'a mask grid of shape (res^3, {a.enc_dim}), contiguous fp32'
    a._cs = (C.c_float * 6)(*[float(v) for v in (IDENTITY_SCALE if centre_scale is None else centre_scale)])
    return ptr(grid), res, C.cast(a._cs, C.c_void_p)


def _out_tensor(given, shape, device):
    """a caller's output tensor of that shape (contiguous fp32 on the GPU), or a new one"""
    t = torch.empty(shape, device=device, dtype=torch.float32) if given is None else given
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape)
    return t


def _call(a, mask=None, enc_grad=False, enc_workspace=None, g_enc_a=None, pose_grad=False, pose_workspace=None, g_poses=None):
    """the call descriptor of a finished network descriptor `a`: what the call takes beside it, one clause per mode bit.  The dimension and
    the pose list are the descriptor's (`_args` / `_siren_args`), `mask` a Mask that is `.spatial` (or None), `enc_grad` / `pose_grad` the
    extra gradients of a backward call, with the caller's buffers or new ones.  `c._g_enc` / `c._g_poses` are those outputs; `c._keep` holds
    every tensor the descriptor points into, for as long as the descriptor lives"""
    c = _lib.FlowNetCall(domain_dim=a._dim)
    c._g_enc = c._g_poses = None
    if a._poses is not None:
        c.mode |= _lib.AT_POINTS
        c.poses, c.n = a._poses
    if mask is not None and mask.spatial:
        c.mode |= _lib.SPATIAL
        c.grid, c.res, c.centre_scale = _spatial(a, mask.tensor, mask.res, mask.centre_scale)
    if pose_grad:
        if a._dim != 3:
            flowcaps.refuse(flowcaps.PAIR_MODES, 'pose_grad', f'domain_dim {a._dim}')
        assert enc_workspace is None, 'with pose_grad the frequency gradient\'s workspace is part of pose_workspace'
        c.mode |= _lib.POSEGRAD
        c._g_poses = _out_tensor(g_poses, (a.W, 3), a._device)
        c.g_poses = ptr(c._g_poses)
        if isinstance(a, _lib.FlowNetArgs):              # SIREN's posegrad call takes no extra workspace
            if pose_workspace is None:
                nbytes = _lib.lib().sininn_flownet_posegrad_workspace_bytes(C.byref(a), int(enc_grad))
                pose_workspace = torch.empty(nbytes // 4, device=a._device, dtype=torch.float32)
            c.extra_workspace, c.extra_workspace_bytes = ptr(pose_workspace), pose_workspace.numel() * 4
    if enc_grad:
        c.mode |= _lib.ENCGRAD
        c._g_enc = _out_tensor(g_enc_a, (3, 256), a._device)
        c.g_enc_a = ptr(c._g_enc)
        if not pose_grad:
            if enc_workspace is None:
                nbytes = _lib.lib().sininn_flownet_encgrad_workspace_bytes(C.byref(a))
                enc_workspace = torch.empty(nbytes // 4, device=a._device, dtype=torch.float32)
            c.enc_workspace, c.enc_workspace_bytes = ptr(enc_workspace), enc_workspace.numel() * 4
    c._keep = (mask, enc_workspace, pose_workspace)
    return c


# ---- the two halves every call shares: a = a finished descriptor, `stem` its family of entry points (sininn_<stem>_forward / _backward),
# c = its call descriptor ----
def _forward(a, train, saved, saved_shape, stem, c):
    """allocate flows and (train) `saved` of `saved_shape()`, call, return (flows, saved); at a pose list flows is the planar (4, N)"""
    flows = torch.empty(a.T, 4, a.H, a.W, device=a._device, dtype=torch.float32)
    a.flows = ptr(flows)
    if train:
        if saved is None:
            saved = torch.empty(saved_shape(), device=a._device, dtype=torch.float32)
        assert saved.is_cuda and saved.is_contiguous() and saved.dtype == torch.float32
        a.saved, a.saved_bytes = ptr(saved), saved.numel() * 4
    else:
        saved = None
    check(getattr(_lib.lib(), f'sininn_{stem}_forward')(C.byref(a), C.byref(c), _stream()))
    return (flows.view(4, -1) if a._poses is not None else flows), saved


def _backward(a, net, dflows, saved, workspace, stem, c, entry=None):
    """the backward half (`entry(a, c)`: the library call to make instead of sininn_<stem>_backward, on the same descriptors): check dflows (at a pose list: (4, N)), allocate the workspace (sininn_<stem>_workspace_bytes(N)) and the gradients
    into the descriptor, call.  [gW1, gb1, ..]; with the frequency gradient (grads, gF); with the pose gradient (either of those, g_poses)"""
    lib = _lib.lib()
    _on_gpu(dflows)
    dflows = (dflows.reshape(1, 4, 1, -1) if a._poses is not None else dflows).contiguous()
    assert tuple(dflows.shape) == (a.T, 4, a.H, a.W) and dflows.dtype == torch.float32
    if workspace is None:
        workspace = torch.empty(getattr(lib, f'sininn_{stem}_workspace_bytes')(a.T * a.H * a.W) // 4, device=a._device, dtype=torch.float32)
    a.saved, a.saved_bytes = ptr(saved), saved.numel() * 4
    a.workspace, a.workspace_bytes = ptr(workspace), workspace.numel() * 4
    a.dflows = ptr(dflows)
    grads = []
    for l, lin in enumerate(net.linears()):
        gw, gb = torch.empty_like(lin.weight), torch.empty_like(lin.bias)
        a.gw[l], a.gb[l] = ptr(gw), ptr(gb)
        grads += [gw, gb]
    if entry is not None:
        check(entry(a, c))
    else:
        check(getattr(lib, f'sininn_{stem}_backward')(C.byref(a), C.byref(c), _stream()))   # dflows, workspace: alive until the call is made
    out = grads if c._g_enc is None else (grads, c._g_enc)
    return out if c._g_poses is None else (out, c._g_poses)


def _flownet_saved_shape(a):
    return lambda: (3, _lib.lib().sininn_flownet_saved_bytes(a.T * a.H * a.W) // (3 * 256 * 4), 256)


def _siren_saved_shape(a):
    return lambda: _lib.lib().sininn_siren_saved_bytes(a.T * a.H * a.W) // 4


def _pack_workspace(a):
    """a progressive forward call under a global mask: the workspace of the packed, masked copy of W1"""
    if a.progressive:
        a._pack = torch.empty(_lib.lib().sininn_flownet_forward_workspace_bytes(C.byref(a)) // 4, device=a._device, dtype=torch.float32)
        a.workspace, a.workspace_bytes = ptr(a._pack), a._pack.numel() * 4
    return a


# ---- the public calls: `times, ys, xs` a grid of points, or (the `_points` forms) a pose list (N, domain_dim) with planar flows / dflows
# (4, N); a global mask or none, or (the `_spatial` forms) a per-point mask from a grid.  Each builds its descriptor and its call
# descriptor and names the family ----
def flownet_forward(net, times, ys, xs, scale, train, saved=None, mask=None, k_active=None, enc_a=None):
    """flows (t, 4, h, w) = net(meshgrid(times, ys, xs)) * scale, and (train) the saved hidden layers as a
    (3, Npad, 256) tensor -- the post-ReLU activations, so `saved > 0` are the gates the kernel took (`saved`: optional
    caller-provided buffer of that shape).  Progressive networks: `mask` is a device tensor of 515 floats (PPE: 27) and `k_active` a
    number of leading features after which the mask is all zero (None: 515, nothing is skipped).  `enc_a`: the frequency matrix
    (3, 256) to use instead of the encoding's own (learnable encodings: F_eff; None: computed here).  Two coordinates: `times` is None,
    the axes are (ys, xs)."""
    a = _pack_workspace(_args(net, times, ys, xs, scale, mask, k_active, enc_a))
    return _forward(a, train, saved, _flownet_saved_shape(a), 'flownet', _call(a))


def flownet_backward(net, times, ys, xs, scale, dflows, saved, workspace=None, mask=None, k_active=None, enc_a=None, enc_grad=False,
                     enc_workspace=None, g_enc_a=None):
    """[gW1, gb1, .., gW4, gb4] for an upstream gradient dflows (t, 4, h, w); `workspace`: optional fp32 tensor of at least
    sininn_flownet_workspace_bytes(N) bytes (allocated here otherwise); `mask` / `k_active` / `enc_a`: those of the forward call.
    `enc_grad=True` (Fourier encodings) returns ([gW1, .., gb4], gF) with gF (3, 256) the gradient with respect to the frequency
    matrix the kernels read; `enc_workspace`: optional fp32 tensor of sininn_flownet_encgrad_workspace_bytes bytes for it,
    `g_enc_a`: optional (3, 256) fp32 tensor that receives gF."""
    a = _args(net, times, ys, xs, scale, mask, k_active, enc_a)
    return _backward(a, net, dflows, saved, workspace, 'flownet', _call(a, None, enc_grad, enc_workspace, g_enc_a))


def flownet_forward_spatial(net, times, ys, xs, scale, train, grid, res, centre_scale=None, k_active=None, saved=None, enc_a=None):
    """flownet_forward under a per-point mask: `grid` (res^3, 515) on the device, the controller's blurred mask; `centre_scale`: six
    host floats, centre (t, y, x) then scale (t, y, x), None: identity; `k_active`: every grid column from there on is zero (None:
    515).  No workspace: W1 is read in place."""
    a = _args(net, times, ys, xs, scale, None, k_active, enc_a, spatial=True)
    return _forward(a, train, saved, _flownet_saved_shape(a), 'flownet', _call(a, Mask(grid, k_active, res, centre_scale)))


def flownet_backward_spatial(net, times, ys, xs, scale, dflows, saved, grid, res, centre_scale=None, k_active=None, workspace=None,
                             enc_a=None, enc_grad=False, enc_workspace=None, g_enc_a=None):
    """flownet_backward under the per-point mask of the forward call; the arguments of flownet_backward and flownet_forward_spatial"""
    a = _args(net, times, ys, xs, scale, None, k_active, enc_a, spatial=True)
    return _backward(a, net, dflows, saved, workspace, 'flownet',
                     _call(a, Mask(grid, k_active, res, centre_scale), enc_grad, enc_workspace, g_enc_a))


def flownet_sample_mask(net, times, ys, xs, grid, res, centre_scale=None):
    """the interpolated mask (N, 515) of the grid of points (`ys is None`: of the pose list `times`), bitwise what the spatial kernels
    multiply layer 1's input by"""
    a = _args(net, times, ys, xs, 1.0, spatial=True)
    c = _call(a, Mask(grid, None, res, centre_scale))
    out = torch.empty(a.T * a.H * a.W, a.enc_dim, device=a._device, dtype=torch.float32)
    check(_lib.lib().sininn_flownet_sample_mask(C.byref(a), C.byref(c), ptr(out), _stream()))
    return out


def siren_forward(net, times, ys, xs, scale, train, saved=None, omega=None):
    """flows (t, 4, h, w) = net(meshgrid(times, ys, xs)) * scale for a SirenModel, and (train) what the backward call needs as one
    opaque fp32 tensor of sininn_siren_saved_bytes(N) bytes (`saved`: optional caller-provided buffer of that size).  `omega`:
    instead of the network's own omega_0 (None)."""
    a = _siren_args(net, times, ys, xs, scale, omega)
    return _forward(a, train, saved, _siren_saved_shape(a), 'siren', _call(a))


def siren_backward(net, times, ys, xs, scale, dflows, saved, workspace=None, omega=None):
    """[gW1, gb1, .., gW5, gb5] for an upstream gradient dflows (t, 4, h, w); `saved`: that of the forward call on the same weights
    and omega; `workspace`: optional fp32 tensor of at least sininn_siren_workspace_bytes(N) bytes (allocated here otherwise)."""
    a = _siren_args(net, times, ys, xs, scale, omega)
    return _backward(a, net, dflows, saved, workspace, 'siren', _call(a))


def flownet_forward_points(net, poses, scale, train, saved=None, mask=None, k_active=None, enc_a=None):
    """flownet_forward at a pose list (N, 3) on the device (two coordinates: (N, 2), columns (y, x)): flows (4, N) = net(poses)^T * scale;
    `saved` as there, for N points"""
    return flownet_forward(net, poses, None, None, scale, train, saved, mask, k_active, enc_a)


def flownet_backward_points(net, poses, scale, dflows, saved, workspace=None, mask=None, k_active=None, enc_a=None, enc_grad=False,
                            enc_workspace=None, g_enc_a=None, pose_grad=False, pose_workspace=None, g_poses=None):
    """flownet_backward at the pose list of the forward call, dflows (4, N); everything else as there.  `pose_grad=True` returns
    (what the call returns without it, g_poses): g_poses (N, 3), the gradient with respect to the coordinates, from the POSEGRAD mode of
    sininn_flownet_backward, which computes everything else as well (bitwise the same); `pose_workspace`: optional fp32
    tensor of sininn_flownet_posegrad_workspace_bytes bytes (it holds the frequency gradient's workspace too: `enc_workspace` is refused),
    `g_poses`: optional (N, 3) fp32 tensor that receives the gradient"""
    a = _args(net, poses, None, None, scale, mask, k_active, enc_a)
    return _backward(a, net, dflows, saved, workspace, 'flownet',
                     _call(a, None, enc_grad, enc_workspace, g_enc_a, pose_grad, pose_workspace, g_poses))


def flownet_forward_spatial_points(net, poses, scale, train, grid, res, centre_scale=None, k_active=None, saved=None, enc_a=None):
    """flownet_forward_points under the per-point mask of flownet_forward_spatial: flows (4, N)"""
    return flownet_forward_spatial(net, poses, None, None, scale, train, grid, res, centre_scale, k_active, saved, enc_a)


def flownet_backward_spatial_points(net, poses, scale, dflows, saved, grid, res, centre_scale=None, k_active=None, workspace=None, enc_a=None,
                                    enc_grad=False, enc_workspace=None, g_enc_a=None, pose_grad=False, pose_workspace=None, g_poses=None):
    """flownet_backward_points under the per-point mask of the forward call, dflows (4, N); `pose_grad=True` as there: the mask is a
    constant of the point, there is no d mask / d pose term"""
    a = _args(net, poses, None, None, scale, None, k_active, enc_a, spatial=True)
    return _backward(a, net, dflows, saved, workspace, 'flownet',
                     _call(a, Mask(grid, k_active, res, centre_scale), enc_grad, enc_workspace, g_enc_a, pose_grad, pose_workspace, g_poses))


def flownet_sample_mask_points(net, poses, grid, res, centre_scale=None):
    """the interpolated mask (N, 515) at a pose list (N, 3), bitwise what the spatial kernels multiply layer 1's input by"""
    return flownet_sample_mask(net, poses, None, None, grid, res, centre_scale)


def siren_forward_points(net, poses, scale, train, saved=None, omega=None):
    """siren_forward at a pose list (N, 3) on the device: flows (4, N)"""
    return siren_forward(net, poses, None, None, scale, train, saved, omega)


def siren_backward_points(net, poses, scale, dflows, saved, workspace=None, omega=None, pose_grad=False, g_poses=None):
    """siren_backward at the pose list of the forward call, dflows (4, N).  `pose_grad=True` returns (the gradients, g_poses (N, 3)),
    from the POSEGRAD mode of sininn_siren_backward"""
    a = _siren_args(net, poses, None, None, scale, omega)
    return _backward(a, net, dflows, saved, workspace, 'siren', _call(a, pose_grad=pose_grad, g_poses=g_poses))


def _functions(net, mask, enc_a, points):
    """(forward, backward, the keyword arguments both take) of a call: a SirenModel, a per-point mask, or a global mask / none; on a grid
    or at a pose list"""
    if isinstance(net, SirenModel):
        return (siren_forward_points, siren_backward_points, {}) if points else (siren_forward, siren_backward, {})
    if mask.spatial:
        kw = dict(grid=mask.tensor, res=mask.res, centre_scale=mask.centre_scale, k_active=mask.k_active, enc_a=enc_a)
        return (flownet_forward_spatial_points, flownet_backward_spatial_points, kw) if points else (flownet_forward_spatial, flownet_backward_spatial, kw)
    kw = dict(mask=mask.tensor, k_active=mask.k_active, enc_a=enc_a)
    return (flownet_forward_points, flownet_backward_points, kw) if points else (flownet_forward, flownet_backward, kw)


def _fields_forward(ctx, name, net, where, scale, train, mask, enc_a, enc_slot, pose_slot=None):
    """the forward half of `_FlowFields` (where = (times, ys, xs)) and `_FlowAt` (where = (poses,)): choose the functions, call, and note
    what the backward half needs; `enc_slot` / `pose_slot`: the positions of enc_a / the poses among the autograd inputs"""
    if enc_a is not None:
        enc_a = enc_a.detach().contiguous()
    forward, ctx.backward_fn, ctx.kw = _functions(net, mask, enc_a, points=len(where) == 1)
    flows, saved = forward(net, *where, scale, train, **ctx.kw)
    ctx.name, ctx.net, ctx.where, ctx.scale, ctx.saved, ctx.mask = name, net, where, scale, saved, mask
    if mask.spatial:
        ctx.grid_version = mask.tensor._version          # the controller updates its grid in place
    if enc_a is not None and ctx.needs_input_grad[enc_slot]:
        ctx.kw['enc_grad'] = True
    if pose_slot is not None and ctx.needs_input_grad[pose_slot]:
        ctx.kw['pose_grad'] = True
    return flows


def _fields_backward(ctx, dflows):
    """the backward half of both: (the parameters' gradients, g_enc or None, g_poses or None)"""
    if ctx.saved is None:
        raise RuntimeError(f'{ctx.name}: backward through an inference-mode forward')
    if ctx.mask.spatial and ctx.mask.tensor._version != ctx.grid_version:
        raise RuntimeError(f'{ctx.name}: the mask grid changed between the forward and the backward pass (run backward before '
                           'the controller\'s next stash_iteration / update_progress: its grid is updated in place)')
    grads, g_enc, g_poses = ctx.backward_fn(ctx.net, *ctx.where, ctx.scale, dflows, ctx.saved, **ctx.kw), None, None
    if ctx.kw.get('pose_grad'):
        grads, g_poses = grads
    if ctx.kw.get('enc_grad'):
        grads, g_enc = grads
    ctx.saved = None
    return tuple(grads), g_enc, g_poses


class _FlowFields(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, times, ys, xs, scale, train, mask, enc_a, *params):
        return _fields_forward(ctx, 'flow_fields', net, (times, ys, xs), scale, train, mask, enc_a, 7)

    @staticmethod
    def backward(ctx, dflows):
        grads, g_enc, _ = _fields_backward(ctx, dflows)
        return (None,) * 7 + (g_enc,) + grads


class _SirenFields:
    """the call `_FlowFields` had for a SirenModel before the two were one function: no mask, no frequency matrix"""

    @staticmethod
    def apply(net, times, ys, xs, scale, train, *params):
        return _FlowFields.apply(net, times, ys, xs, scale, train, Mask(), None, *params)


class _FlowAt(torch.autograd.Function):
    """`_FlowFields` at a pose list: flows (4, N).  `pose_grad` and poses that require it: the backward pass is the posegrad call and
    returns the gradient of the coordinates as well.  Once differentiable: the gradients come from kernels, a double backward raises"""

    @staticmethod
    def forward(ctx, net, poses, scale, train, mask, enc_a, pose_grad, *params):
        return _fields_forward(ctx, 'flow_at', net, (poses,), scale, train, mask, enc_a, 5, 1 if pose_grad else None)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dflows):
        grads, g_enc, g_poses = _fields_backward(ctx, dflows)
        return (None, g_poses, None, None, None, g_enc, None) + grads


# ---- the Jacobian as an output: d flow / d (t, y, x) at a pose list, with a gradient to the parameters (csrc/flownet_jacobian.h) ----
JACOBIAN_AXES = 'tyx'


def jacobian_dirs(jacobian):
    """the direction set of a `jacobian=` keyword as indices into (t, y, x), ascending: a string of distinct letters from 'tyx', True: 'yx'"""
    if jacobian is True:
        jacobian = 'yx'
    if not isinstance(jacobian, str) or not jacobian or len(set(jacobian)) != len(jacobian) or any(ch not in JACOBIAN_AXES for ch in jacobian):
        raise ValueError(f'jacobian: a non-empty string of distinct letters from {JACOBIAN_AXES!r} (True: \'yx\'); got {jacobian!r}')
    return tuple(d for d, ch in enumerate(JACOBIAN_AXES) if ch in jacobian)


def _refuse_jacobian(net, override_mask=None, pose_grad=False, poses=None, what='flow_at(.., jacobian=)'):
    """what the Jacobian kernels do not do, each refusal a ValueError that names what is missing; `net`: a model or a controller.  Needs no
    device"""
    from .progressive import StashedSpatialController
    model, row = _row(net)
    flowcaps.refuse(row, 'jacobian', what)
    if model.domain_dim != 3:
        raise ValueError(f'{what}: domain_dim {model.domain_dim} is out of scope: the Jacobian kernels take three coordinates (t, y, x)')
    if isinstance(net, StashedSpatialController) or (override_mask is not None and override_mask.dim() == 2):
        raise ValueError(f'{what}: per-point (spatial) masks are out of scope: the tangent passes read the mask-folded layer 1 of a global mask')
    if pose_grad:
        raise ValueError(f'{what}: pose_grad=True cannot be combined with the Jacobian: there is no gradient to the poses through it')
    if poses is not None and poses.requires_grad:
        raise ValueError(f'{what}: poses that require a gradient: there is no gradient to the poses through the Jacobian (poses.detach())')


def _dirs_bits(dirs):
    return sum(1 << d for d in dirs)


def flownet_jacobian_forward_points(net, poses, scale, dirs, mask=None, k_active=None):
    """(flows (4, N), jac (|D|, 4, N), saved, tsaved) at a pose list (N, 3): sininn_flownet_jacobian_forward.  `dirs`: ascending indices into
    (t, y, x).  flows and `saved` are bitwise those of flownet_forward_points(.., train=True); jac[i] = scale d out / d x_dirs[i]; tsaved
    (|D|, 3, Npad, 256) holds the gated tangents for the backward call"""
    a = _pack_workspace(_args(net, poses, None, None, scale, mask, k_active))
    c = _call(a)
    lib, n, nd = _lib.lib(), a.W, len(dirs)
    flows = torch.empty(1, 4, 1, n, device=a._device, dtype=torch.float32)
    saved = torch.empty(_flownet_saved_shape(a)(), device=a._device, dtype=torch.float32)
    jac = torch.empty(nd, 4, n, device=a._device, dtype=torch.float32)
    tsaved = torch.empty((nd,) + tuple(saved.shape), device=a._device, dtype=torch.float32)
    a.flows, a.saved, a.saved_bytes = ptr(flows), ptr(saved), saved.numel() * 4
    check(lib.sininn_flownet_jacobian_forward(C.byref(a), C.byref(c), _dirs_bits(dirs), ptr(jac), ptr(tsaved), tsaved.numel() * 4, _stream()))
    return flows.view(4, -1), jac, saved, tsaved


def flownet_jacobian_backward_points(net, poses, scale, dirs, dflows, djac, saved, tsaved, workspace=None, jac_workspace=None, mask=None,
                                     k_active=None):
    """[gW1, gb1, .., gW4, gb4] of sum(dflows * flows) + sum(djac * jac): sininn_flownet_jacobian_backward.  dflows (4, N), djac (|D|, 4, N);
    with djac all zero the gradients are bitwise flownet_backward_points'.  `jac_workspace`: optional fp32 tensor of
    sininn_flownet_jacobian_workspace_bytes bytes"""
    a = _args(net, poses, None, None, scale, mask, k_active)
    lib, n, nd = _lib.lib(), a.W, len(dirs)
    _on_gpu(djac)
    djac = djac.contiguous()
    assert tuple(djac.shape) == (nd, 4, n) and djac.dtype == torch.float32
    if jac_workspace is None:
        jac_workspace = torch.empty(lib.sininn_flownet_jacobian_workspace_bytes(C.byref(a), n, nd) // 4, device=a._device, dtype=torch.float32)

    def entry(a, c):
        return lib.sininn_flownet_jacobian_backward(C.byref(a), C.byref(c), _dirs_bits(dirs), ptr(djac), ptr(tsaved), tsaved.numel() * 4,
                                                    ptr(jac_workspace), jac_workspace.numel() * 4, _stream())
    return _backward(a, net, dflows, saved, workspace, 'flownet', _call(a), entry)


class _FlowJacobianAt(torch.autograd.Function):
    """(flows (4, N), jac (|D|, 4, N)) of one call; both carry a gradient to the parameters.  Once differentiable; an upstream of None for
    either output is a zero"""

    @staticmethod
    def forward(ctx, net, poses, scale, train, mask, dirs, *params):
        kw = dict(mask=mask.tensor, k_active=mask.k_active)
        flows, jac, saved, tsaved = flownet_jacobian_forward_points(net, poses, scale, dirs, **kw)
        ctx.net, ctx.poses, ctx.scale, ctx.dirs, ctx.kw = net, poses, scale, dirs, kw
        ctx.saved, ctx.tsaved = (saved, tsaved) if train else (None, None)
        return flows, jac

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dflows, djac):
        if ctx.saved is None:
            raise RuntimeError('flow_at(.., jacobian=): backward through an inference-mode forward')
        if dflows is None:
            dflows = torch.zeros(4, ctx.poses.shape[0], device=ctx.poses.device)
        if djac is None:                                 # the flows alone: the plain backward call
            grads = flownet_backward_points(ctx.net, ctx.poses, ctx.scale, dflows, ctx.saved, **ctx.kw)
        else:
            grads = flownet_jacobian_backward_points(ctx.net, ctx.poses, ctx.scale, ctx.dirs, dflows, djac, ctx.saved, ctx.tsaved, **ctx.kw)
        ctx.saved = ctx.tsaved = None
        return (None,) * 6 + tuple(grads)


def _encoding_with_tangents(enc, x, dirs):
    """(E (N, 512), [dE_d (N, 512) for d in dirs]) of a RadialBasisEncoding / a fixed Fourier encoding in x's dtype, torch ops"""
    if enc.kind == RBF:
        centres, s2 = enc.centres.to(x), enc.sigma.to(x)[None, :] ** 2
        diff = x[:, None, :] - centres[None, :, :]
        e = torch.exp(-(diff.pow(2).sum(2) * s2))
        return e, [(-2 * s2) * diff[:, :, d] * e for d in dirs]
    freq = enc.frequencies.to(x)
    phi = torch.matmul(x * 2 * math.pi, freq)
    sn, co = torch.sin(phi), torch.cos(phi)
    e = torch.stack((sn, co), dim=2).view(x.shape[0], -1)
    return e, [torch.stack(((2 * math.pi * freq[d])[None, :] * co, (-2 * math.pi * freq[d])[None, :] * sn), dim=2).view(x.shape[0], -1)
               for d in dirs]


def flow_jacobian_composed(net, poses, scale=1.0, jacobian='yx', override_mask=None, planar=False, gates=None):
    """(flow, jac) as flow_at(net, poses, scale, jacobian=..) returns them, from torch ops on any device in the dtype of `poses` (fp32 or
    fp64): the value pass of the module, then one forward-mode tangent pass per direction under the value pass's own ReLU decisions,
    no bias, the tangent of cat((t, y, x), enc) = (e_d, dE_d).  Differentiable with respect to the parameters by ordinary autograd (the gates
    carry no gradient).  The baseline of the fused call and the CPU path.  `gates`: three bool (N, 256) tensors that replace the ReLU
    decisions (the tests force the kernel's own)"""
    dirs = jacobian_dirs(jacobian)
    _refuse_jacobian(net, override_mask, what='flow_jacobian_composed')
    if not torch.is_tensor(poses) or poses.dim() < 1 or poses.shape[-1] != 3 or poses.dtype not in (torch.float32, torch.float64):
        raise ValueError('flow_jacobian_composed: poses of shape (..., 3), fp32 or fp64')
    lead = poses.shape[:-1]
    x = poses.detach().reshape(-1, 3)
    from .progressive import ProgressiveEncoderController
    model = net.model if isinstance(net, ProgressiveEncoderController) else net
    e, de = _encoding_with_tangents(model.encode, x, dirs)
    if model.is_progressive:
        # the mask of the call, as _resolve_mask chooses it, read where it lives (a controller keeps its own on the host)
        m = override_mask if override_mask is not None else net.mask if model is not net else torch.ones(model.encoding_dim)
        m = m.detach().to(x)[None, :]
        e = torch.cat((x, e), dim=1) * m
        unit = torch.eye(3, dtype=x.dtype, device=x.device)
        de = [torch.cat((unit[d][None, :].expand(x.shape[0], 3), t), dim=1) * m
              for d, t in zip(dirs, de)]
    lins = model.linears()
    h, ts = e, de
    for l in range(3):
        w, b = lins[l].weight.to(x.dtype), lins[l].bias.to(x.dtype)
        pre = nnf.linear(h, w, b)
        g = ((pre > 0) if gates is None else gates[l]).to(x.dtype)
        h = pre * g
        ts = [nnf.linear(t, w) * g for t in ts]
    w, b = lins[3].weight.to(x.dtype), lins[3].bias.to(x.dtype)
    flow = nnf.linear(h, w, b) * scale
    jac = torch.stack([nnf.linear(t, w) * scale for t in ts], dim=0)          # (|D|, N, 4)
    if planar:
        return flow.t().contiguous(), jac.permute(0, 2, 1).contiguous()
    return flow.view(*lead, 4), jac.permute(1, 2, 0).contiguous().view(*lead, 4, len(dirs))


def grid_axes(net, times, h, w):
    """linspace(-1, 1, h) / (w) as trainer.py:40-41 makes them: on the CPU, then moved next to `times` (bit-identical
    coordinates); cached per size and device."""
    key = (h, w, times.device)
    if key not in net._axes:
        net._axes[key] = (torch.linspace(-1, 1, h).to(times), torch.linspace(-1, 1, w).to(times))
    return net._axes[key]


def last_open(mask):
    """k_active of a HOST mask: the number of leading features after which every entry is zero"""
    nz = torch.nonzero(mask).reshape(-1)
    return int(nz[-1]) + 1 if nz.numel() else 0


def _resolve_mask(net, override_mask, device):
    """(model, Mask) for a plain model (no mask), a bare progressive model (all ones) or a controller (a module that wraps a
    progressive model as `.model` and keeps a mask); a grid under a spatial controller or a raw 2-D `override_mask`"""
    from .progressive import ProgressiveEncoderController, StashedSpatialController
    controller = net if isinstance(net, ProgressiveEncoderController) else None
    spatial = controller if isinstance(controller, StashedSpatialController) else None
    model = net.model if controller is not None else net
    if not model.is_progressive:
        if override_mask is not None:
            raise ValueError('override_mask needs a progressive network')
        return model, Mask()
    if override_mask is not None and override_mask.dim() == 2:            # three coordinates: _call_dim has refused a grid at two
        # a raw grid (res^3, enc_dim) on the device: not inspected, nothing skipped; the cell map is the spatial controller's, else identity
        g = override_mask.detach()
        _on_gpu(g, 'mask grid')
        res = round(g.shape[0] ** (1.0 / 3.0))
        if res ** 3 != g.shape[0] or g.shape[1] != model.encoding_dim:
            raise ValueError(f'a mask grid has shape (res^3, {model.encoding_dim}); got {tuple(g.shape)}')
        cs = spatial.centre_scale_host() if spatial is not None else IDENTITY_SCALE
        return model, Mask(g.to(device=device, dtype=torch.float32).contiguous(), model.encoding_dim, res, cs)
    if override_mask is not None:
        m = override_mask.detach()
        assert m.dim() == 1 and m.numel() == model.encoding_dim, 'a global mask of encoding_dim values, or a grid (res^3, encoding_dim)'
        if m.is_cuda:                                    # not inspected on the host: no synchronisation, nothing skipped
            return model, Mask(m.to(device=device, dtype=torch.float32).contiguous(), model.encoding_dim)
        m = m.to(torch.float32).contiguous()
        return model, Mask(m.to(device), last_open(m))
    if spatial is not None:
        return model, spatial.device_grid(device)
    if controller is not None:
        return model, controller.device_mask(device)
    return model, Mask(model.ones_mask(device), model.encoding_dim)


def flow_fields(net, times, h, w, scale, override_mask=None, get_mask=False):
    """FlowTrainer.forward (trainer.py:37-45): (flow12, flow21), each (t, 2, h, w), views of one (t, 4, h, w) tensor.  Under
    torch.no_grad() (or with no trainable parameter) the inference mode of the kernel runs and nothing is saved.  `net` is a
    model or a controller around a progressive model; `override_mask` (515 values, PPE: 27; progressive networks only) replaces the
    controller's mask.  A learnable encoding (RFF / PRFF) contributes F_eff, computed here with torch ops; its gradient is computed
    only if `encode.frequencies` requires one.  A SirenModel runs in its own kernels under the same contract.
    A StashedSpatialController, or an `override_mask` of shape (res^3, 515) on the device, evaluates the network under the per-point
    mask interpolated from that grid.  `get_mask=True` (the reference's keyword) returns (flow12, flow21, mask): the mask in use, (515,)
    or, spatial, the interpolated (t h w, 515)."""
    dim = _call_dim(net, override_mask)
    if dim == 2:
        # one frame pair (pair_flow.py:55-59): poses linspace(-1, 1, h) x linspace(-1, 1, w), no time axis; flows (1, 4, h, w)
        if times is not None:
            raise ValueError('domain_dim 2: `times` given for a network on (y, x): flow_fields(net, None, h, w, scale) evaluates one frame pair')
        like = next(net.parameters())
        _on_gpu(like, 'parameter')
    else:
        if times is None:
            raise ValueError(f'domain_dim {dim}: times=None is the call of a network on (y, x) (domain_dim 2); this one needs its times')
        _on_gpu(times)
        assert times.dtype == torch.float32 and times.dim() == 1
        like = times
    controller = net
    net, mask = _resolve_mask(net, override_mask, like.device)
    ys, xs = grid_axes(net, like, h, w)
    if mask.spatial and hasattr(controller, 'note_grid'):
        controller.note_grid(times, ys, xs)              # stash_iteration finds the cells of these points
    if get_mask:
        if not net.is_progressive:
            raise ValueError('get_mask needs a progressive network')
        used = mask.tensor
        if mask.spatial:
            with torch.no_grad():
                used = flownet_sample_mask(net, times, ys, xs, mask.tensor, mask.res, mask.centre_scale)
        return (*flow_fields(controller, times, h, w, scale, override_mask), used)
    params = [p for lin in net.linears() for p in (lin.weight, lin.bias)]
    enc_a = net.encode.effective_frequencies() if isinstance(getattr(net, 'encode', None), RotatedFourierFeatures) else None
    train = torch.is_grad_enabled() and (any(p.requires_grad for p in params) or (enc_a is not None and enc_a.requires_grad))
    flows = _FlowFields.apply(net, times, ys, xs, float(scale), train, mask, enc_a, *params)
    return flows[:, :2], flows[:, 2:]


def flow_at(net, poses, scale=1.0, override_mask=None, get_mask=False, planar=False, pose_grad=False, jacobian=None):
    """net(poses) * scale (trainer.py:43-44, progressive_controller.py:45-53) at arbitrary points: `poses` (..., 3) fp32 on the GPU,
    columns (t, y, x) -> (..., 4), contiguous.  `net`: what flow_fields takes, a model or a LinearController / LinearControllerEarly
    around a progressive one; `override_mask` (515 values, PPE: 27) replaces the controller's mask.  A StashedSpatialController, or a
    controller with an `override_mask` of shape (res^3, 515) on the device, evaluates the network under the per-point mask interpolated from
    that grid (the mask is a constant of the point: `pose_grad` has no d mask / d pose term), and `get_mask=True` returns the interpolated
    mask (..., 515) then.  The kernels read the list in place
    and write the planar (4, N) layout; `planar=True` returns that tensor, without the transpose to the reference's layout.
    Differentiable with respect to the parameters (and `encode.frequencies` of RFF / PRFF); under torch.no_grad() (or with no trainable
    parameter) the inference mode runs and nothing is saved.  `get_mask=True` returns (out, the mask in use on the device).
    `pose_grad=True`: poses that require a gradient get one (d flow / d pose against the upstream gradient, `scale` included, computed
    by the fused kernels: the POSEGRAD mode of sininn_flownet_backward / sininn_siren_backward), which chains queries:
    flow_at(net, p + pad(flow_at(net, p, pose_grad=True)[..., :2]), pose_grad=True).  Once differentiable.  Without the keyword there is no
    gradient with respect to the coordinates: poses that require one are refused.
    `jacobian`: a string of distinct letters from 'tyx' (True: 'yx') returns (out, jac): jac (..., 4, |D|) (`planar=True`: (|D|, 4, N)), the
    derivative of `out` along each named coordinate, always in the order t, y, x, in flow units (`scale` included) per unit of the normalised
    coordinate.  `out` is bitwise the call's without the keyword, and BOTH carry a gradient to the parameters (one autograd function, the
    tangent kernels of csrc/flownet_jacobian.h), so a loss on the derivative trains.  The networks with the table's `jacobian` (flowcaps.py)
    under a global mask; everything else, `pose_grad=True`, poses that require a gradient and `get_mask` with it are refused with a ValueError."""
    dirs = None
    if jacobian is not None and jacobian is not False:
        dirs = jacobian_dirs(jacobian)
        _refuse_jacobian(net, override_mask, pose_grad, poses if torch.is_tensor(poses) else None)
        if get_mask:
            raise ValueError('flow_at(.., jacobian=): get_mask cannot be combined with the Jacobian; ask for the mask in a call of its own')
    dim = _call_dim(net, override_mask, pose_grad)
    if not torch.is_tensor(poses) or poses.dim() < 1 or poses.shape[-1] != dim:
        raise ValueError(f'flow_at: domain_dim {dim}: poses of shape (..., {dim}), columns {"(t, y, x)" if dim == 3 else "(y, x)"}; got '
                         f'{tuple(poses.shape) if torch.is_tensor(poses) else type(poses)}')
    if poses.dtype != torch.float32:
        raise ValueError(f'flow_at: fp32 poses; got {poses.dtype}')
    if poses.requires_grad and not pose_grad:
        raise NotImplementedError('flow_at: there is no gradient with respect to the coordinates unless asked for: pass pose_grad=True, '
                                  'or poses.detach()')
    _on_gpu(poses, 'pose list')
    lead = poses.shape[:-1]
    flat = poses.reshape(-1, dim).contiguous()
    controller = net
    net, mask = _resolve_mask(net, override_mask, poses.device)
    if mask.spatial and controller is net:
        raise NotImplementedError('flow_at: a mask grid at a pose list is a controller\'s (StashedSpatialController, or a linear controller '
                                  'with the grid as override_mask): the interpolation of the grid is the controller\'s in the reference; a '
                                  'bare model takes a grid on a (times, h, w) grid only, with flow_fields')
    if get_mask and not net.is_progressive:
        raise ValueError('get_mask needs a progressive network')
    if mask.spatial and hasattr(controller, 'note_poses'):
        controller.note_poses(flat)                      # stash_iteration finds the cells of these points
    params = [p for lin in net.linears() for p in (lin.weight, lin.bias)]
    enc_a = net.encode.effective_frequencies() if isinstance(getattr(net, 'encode', None), RotatedFourierFeatures) else None
    train = torch.is_grad_enabled() and (any(p.requires_grad for p in params) or (enc_a is not None and enc_a.requires_grad) or
                                         (pose_grad and poses.requires_grad))
    if dirs is not None:
        out, jac = _FlowJacobianAt.apply(net, flat, float(scale), train, mask, dirs, *params)
        if planar:
            return out, jac
        return out.t().contiguous().view(*lead, 4), jac.permute(2, 1, 0).contiguous().view(*lead, 4, len(dirs))
    out = _FlowAt.apply(net, flat, float(scale), train, mask, enc_a, bool(pose_grad), *params)
    if not planar:
        out = out.t().contiguous().view(*lead, 4)
    if get_mask and mask.spatial:
        with torch.no_grad():
            used = flownet_sample_mask_points(net, flat.detach(), mask.tensor, mask.res, mask.centre_scale)
        return out, used.view(*lead, used.shape[-1])
    return (out, mask.tensor) if get_mask else out
