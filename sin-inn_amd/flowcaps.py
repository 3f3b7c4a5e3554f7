"""What each flow network can be asked for: the one table behind the refusals of `flownet`, of the trainer and of the command lines
(DESIGN 25).  A network or a mode is added HERE: the name tuples of the command lines and the Python refusals follow from it.  The C
library keeps refusals of its own (it has other callers).  No torch and no ctypes: video-interpolation/main.py parses its arguments with
this file alone, loaded by path.

A row is a network name of `flownet.flow_model_dict`.  Its capability entries are OK or the reason clause of the refusal: `pair` two
coordinates per point (domain_dim 2), `spatial` per-point masks, `enc_grad` the frequency gradient, `pose_grad` the coordinate gradient,
`jacobian` the Jacobian as an output.  `refuse(row, capability, what)` raises the ValueError under the caller's prefix.  `spatial` and
`enc_grad` are refused by the library itself; no Python refusal prints their clauses, the command line reads them as yes or no.
"""
from collections import namedtuple
from types import SimpleNamespace

RBF, FOURIER, RBFG, PE, PIECEWISE = 0, 1, 3, 4, 5       # the encodings of the kernels (include/sininn.h); siren has none
OK = None
# kind: the encoding the kernels evaluate; progressive: layer 1 reads cat((coordinates, encoding)) under a mask; learnable: the frequencies
# are a parameter; width: inputs of layer 1 at three coordinates; cli: video-interpolation/main.py --net opens it; then the capabilities
Row = namedtuple('Row', 'kind progressive learnable width cli pair spatial enc_grad pose_grad jacobian')

P_RFF = 'RFF / PRFF (learnable frequencies) are out of scope: the frequency gradient exists for three coordinates only'
P_PE = 'PE / PPE are out of scope: 16 features, a layer 1 of another width than the kernels are built for'
P_MPFF = 'MPFF (the piecewise-linear encoding) is out of scope: its kernels take three coordinates'
P_SIREN = 'SIREN is out of scope: its kernels take three coordinates'
J_RFF = 'RFF / PRFF are out of scope: learnable frequencies would need the second derivative of the encoding'
J_RBFG = 'RBFG / PRBFG are out of scope: no tangent kernel exists for the radial-basis grid'
J_PE = 'PE / PPE are out of scope: no tangent kernel exists for the narrow positional layer 1'
J_MPFF = 'MPFF is out of scope: no tangent kernel exists for the piecewise-linear encoding'
J_SIREN = 'SIREN is out of scope: the tangent of a sine layer is no gated copy of the network (no kernel evaluates it)'
S_PLAIN = 'a spatial mask needs a progressive network'
S_PPE = 'PPE is out of scope: the per-point masks are built for the 515-wide progressive networks'
G_NONE = 'the frequency gradient exists for the Fourier encodings only'
T, F = True, False

TABLE = {
    #             kind     progressive learnable width cli  pair  spatial  enc_grad pose_grad jacobian
    'RBF':   Row(RBF,       F, F, 512, T, OK,      S_PLAIN, G_NONE, OK, OK),
    'FFN':   Row(FOURIER,   F, F, 512, T, OK,      S_PLAIN, OK,     OK, OK),
    'UFF':   Row(FOURIER,   F, F, 512, T, OK,      S_PLAIN, OK,     OK, OK),
    'PRBF':  Row(RBF,       T, F, 515, T, OK,      OK,      G_NONE, OK, OK),
    'PFF':   Row(FOURIER,   T, F, 515, T, OK,      OK,      OK,     OK, OK),
    'PUFF':  Row(FOURIER,   T, F, 515, T, OK,      OK,      OK,     OK, OK),
    'RFF':   Row(FOURIER,   F, T, 512, T, P_RFF,   S_PLAIN, OK,     OK, J_RFF),
    'PRFF':  Row(FOURIER,   T, T, 515, T, P_RFF,   OK,      OK,     OK, J_RFF),
    'RBFG':  Row(RBFG,      F, F, 512, T, OK,      S_PLAIN, G_NONE, OK, J_RBFG),
    'PRBFG': Row(RBFG,      T, F, 515, T, OK,      OK,      G_NONE, OK, J_RBFG),
    'PE':    Row(PE,        F, F, 24,  T, P_PE,    S_PLAIN, G_NONE, OK, J_PE),
    'PPE':   Row(PE,        T, F, 27,  T, P_PE,    S_PPE,   G_NONE, OK, J_PE),
    'siren': Row(None,      F, F, 3,   F, P_SIREN, S_PLAIN, G_NONE, OK, J_SIREN),
    'MPFF':  Row(PIECEWISE, T, F, 515, F, P_MPFF,  OK,      G_NONE, OK, J_MPFF),
}
# a model finds its row by what its kernels are, so a class of a caller's own does too; FFN and UFF share every entry that is looked up so
BY_ENCODING = {(row.kind, row.learnable): row for row in TABLE.values()}
# what two coordinates lack whatever the network: read with `refuse` like a row
PAIR_MODES = SimpleNamespace(
    spatial='per-point masks (StashedSpatialController, a 2-D override_mask grid) are out of scope: the mask grid is one over (t, y, x)',
    pose_grad='pose_grad=True is out of scope: the coordinate gradient exists for three coordinates only')


def names(capability=None, cli=None):
    """the network names, in the table's order, that have `capability` and whose `cli` is the one given (None: either)"""
    return tuple(name for name, row in TABLE.items()
                 if (capability is None or getattr(row, capability) is OK) and cli in (None, row.cli))


def refuse(row, capability, what):
    """the ValueError of a capability the row lacks: `what`, the caller's prefix, then the entry's reason clause"""
    reason = getattr(row, capability)
    if reason is not OK:
        raise ValueError(f'{what}: {reason}')


def check_step_options(args, points_max=None, before_smooth=None):
    """The rules of the training step's own options, for both who state them; raises ValueError.  `points_max=None` is the command line
    (main.py get_args): it checks what was typed whatever the weights, and knows no upper bound.  With `points_max` it is
    FlowTrainer.__init__: a term is checked only under a non-zero weight, with every range the step relies on; `before_smooth()` is its
    check of the network, which has always come before the range of --smooth-points."""
    cli = points_max is None

    def on(weight):
        return cli or float(getattr(args, weight, 0) or 0) != 0

    def points(flag, n, per):
        if n < 1 or (not cli and n > points_max):
            raise ValueError(f'{flag} N: N >= 1' if cli else f'{flag} {n}: 1 to {points_max} points a step ({per})')

    if on('loss_between') and not cli:
        taus, back, dt = int(getattr(args, 'between_taus', 1)), getattr(args, 'between_back', 'network'), getattr(args, 'between_dt', None)
        if not 1 <= taus <= 32:
            raise ValueError(f'--between-taus {taus}: 1 to 32 times a step (two rows of one gather call each)')
        if back not in ('network', 'reverse'):
            raise ValueError(f"--between-back is 'network' or 'reverse', got {back!r}")
        if dt is None or not float(dt) > 0:
            raise ValueError('--loss-between needs between_dt, the spacing of the clip\'s times, 2 / (frames - 1)')
    if on('loss_between') and getattr(args, 'between_points', None) is not None:
        if hasattr(args, 'between_taus'):
            raise ValueError('--between-taus draws whole frames, --between-points sampled points: give one of them')
        points('--between-points', int(args.between_points), 'one flow_at call a slab')
    if on('loss_smooth_at'):
        if before_smooth is not None:
            before_smooth()
        n = getattr(args, 'smooth_points', None)
        if not cli or n is not None:
            points('--smooth-points', n if cli else int(n or 4096), 'one flow_at call')       # the trainer reads 0 as "not given"
