"""No GPU needed: the call descriptor of the flow networks (sininn_flownet_call, include/sininn.h) against the 25 entry points it replaced.

tests/golden/flownet_refusals.json was recorded through those 25 symbols, at the commit it names, on a machine without a GPU: for every old
entry point and every defect that applies to it, the full text of sininn_last_error().  `test_every_recorded_refusal_is_unchanged` makes the
same call through the five entry points that remain, with the mode the old name spelled, and compares the text for equality: refusal text is
behaviour.  `test_new_refusals_name_the_combination` covers what only the call descriptor can get wrong.  Every case is refused on the host:
FAKE is never read.
"""
import ctypes as C
import json
import math
import os
import types

import pytest

FAKE = 0x1000                                  # a non-null, 16-byte aligned address that is never read
BIG = 1 << 40
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'flownet_refusals.json')
AT_POINTS, SPATIAL, ENCGRAD, POSEGRAD = 1, 2, 4, 8

# old entry point -> (the entry point that remains, the mode its name spelled, it took the dimension as an argument)
OLD = {
    'sininn_flownet_forward': ('sininn_flownet_forward', 0, False),
    'sininn_flownet_backward': ('sininn_flownet_backward', 0, False),
    'sininn_flownet_forward_dim': ('sininn_flownet_forward', 0, True),
    'sininn_flownet_backward_dim': ('sininn_flownet_backward', 0, True),
    'sininn_flownet_forward_points_dim': ('sininn_flownet_forward', AT_POINTS, True),
    'sininn_flownet_backward_points_dim': ('sininn_flownet_backward', AT_POINTS, True),
    'sininn_flownet_backward_encgrad': ('sininn_flownet_backward', ENCGRAD, False),
    'sininn_flownet_forward_spatial': ('sininn_flownet_forward', SPATIAL, False),
    'sininn_flownet_backward_spatial': ('sininn_flownet_backward', SPATIAL, False),
    'sininn_flownet_backward_encgrad_spatial': ('sininn_flownet_backward', SPATIAL | ENCGRAD, False),
    'sininn_flownet_sample_mask': ('sininn_flownet_sample_mask', SPATIAL, False),
    'sininn_flownet_forward_points': ('sininn_flownet_forward', AT_POINTS, False),
    'sininn_flownet_backward_points': ('sininn_flownet_backward', AT_POINTS, False),
    'sininn_flownet_backward_encgrad_points': ('sininn_flownet_backward', AT_POINTS | ENCGRAD, False),
    'sininn_flownet_backward_posegrad_points': ('sininn_flownet_backward', AT_POINTS | POSEGRAD, False),
    'sininn_flownet_forward_spatial_points': ('sininn_flownet_forward', AT_POINTS | SPATIAL, False),
    'sininn_flownet_backward_spatial_points': ('sininn_flownet_backward', AT_POINTS | SPATIAL, False),
    'sininn_flownet_backward_encgrad_spatial_points': ('sininn_flownet_backward', AT_POINTS | SPATIAL | ENCGRAD, False),
    'sininn_flownet_backward_posegrad_spatial_points': ('sininn_flownet_backward', AT_POINTS | SPATIAL | POSEGRAD, False),
    'sininn_flownet_sample_mask_points': ('sininn_flownet_sample_mask', AT_POINTS | SPATIAL, False),
    'sininn_siren_forward': ('sininn_siren_forward', 0, False),
    'sininn_siren_backward': ('sininn_siren_backward', 0, False),
    'sininn_siren_forward_points': ('sininn_siren_forward', AT_POINTS, False),
    'sininn_siren_backward_points': ('sininn_siren_backward', AT_POINTS, False),
    'sininn_siren_backward_posegrad_points': ('sininn_siren_backward', AT_POINTS | POSEGRAD, False),
}
REMAIN = sorted({new for new, _, _ in OLD.values()})
REMOVED = sorted(set(OLD) - set(REMAIN))


def base(_lib, symbol):
    """a call through `symbol` that nothing refuses: a progressive network (RBF; the encgrad calls: Fourier) on 198 points, every pointer
    FAKE, every size ample.  A namespace: `args` the network descriptor, the rest what the call takes beside it; `mode` is what the
    call descriptor states (the old entry points spelled it in their names, and ENCGRAD beside POSEGRAD by a non-null g_enc_a)"""
    _, mode, takes_dim = OLD[symbol]
    s = types.SimpleNamespace(mode=mode, dim=2 if takes_dim else 3, poses=FAKE, n=198, grid=FAKE, res=3, cs=(C.c_float * 6)(0, 0, 0, 1, 1, 1),
                              g_enc_a=FAKE if mode & ENCGRAD else None, enc_ws=FAKE, enc_ws_bytes=BIG, g_poses=FAKE, extra_ws=FAKE,
                              extra_ws_bytes=BIG, out=FAKE)
    if 'siren' in symbol:
        a = _lib.SirenArgs()
        a.in_dim, a.hidden, a.layers, a.out_dim, a.omega = 3, 256, 3, 4, 30.0
        layers = 5
    else:
        a = _lib.FlowNetArgs()
        a.encoding, a.enc_dim, a.hidden, a.layers, a.out_dim = (1 if mode & ENCGRAD else 0), 512 + s.dim, 256, 3, 4
        a.progressive, a.k_active, a.mask = 1, a.enc_dim, FAKE
        a.enc_a = a.enc_b = FAKE
        layers = 4
    a.T, a.H, a.W, a.scale = (1 if s.dim == 2 else 2), 9, 11, 1.0
    a.times = a.ys = a.xs = a.flows = a.dflows = a.saved = a.workspace = FAKE
    a.saved_bytes = a.workspace_bytes = BIG
    for l in range(layers):
        a.w[l] = a.b[l] = a.gw[l] = a.gb[l] = FAKE
    s.args = a
    return s


def _set(**fields):
    """a defect of the network descriptor"""
    def apply(s):
        for k, v in fields.items():
            setattr(s.args, k, v)
    return apply


def _beside(**fields):
    """a defect of what the call takes beside the network descriptor"""
    def apply(s):
        for k, v in fields.items():
            setattr(s, k, v)
    return apply


def _null_w1(s):
    s.args.w[1] = None


def _off_by_8(s):
    s.args.struct_bytes += 8


def _enc_dim_plus_1(s):
    s.args.k_active = s.args.enc_dim + 1


def _plain(s):
    s.args.progressive, s.args.enc_dim = 0, 512


def _rbf_with_encgrad(s):
    s.args.encoding, s.g_enc_a, s.mode = 0, FAKE, s.mode | ENCGRAD


flownet = lambda y: 'flownet' in y                                   # noqa: E731
siren = lambda y: 'siren' in y                                       # noqa: E731
points = lambda y: 'points' in y                                     # noqa: E731
spatial = lambda y: 'spatial' in y or 'sample_mask' in y             # noqa: E731
sample = lambda y: 'sample_mask' in y                                # noqa: E731
forward = lambda y: 'forward' in y                                   # noqa: E731
backward = lambda y: 'backward' in y                                 # noqa: E731
encgrad = lambda y: 'encgrad' in y                                   # noqa: E731
posegrad = lambda y: 'posegrad' in y                                 # noqa: E731
takes_dim = lambda y: y.endswith('_dim')                             # noqa: E731
packs = lambda y: flownet(y) and forward(y) and not spatial(y)       # the progressive forward call that packs W1 into a workspace

# defect -> (the entry points it applies to, what it does to a base call).  Each is refused before any launch at every entry point it
# applies to, which is what `applies` is for: a null g_enc_a is no defect of a posegrad call, T = 2 none of a points call
DEFECTS = {
    'null args': (lambda y: True, _beside(args=None)),
    'struct_bytes off by 8': (lambda y: True, _off_by_8),
    'hidden 128': (lambda y: True, _set(hidden=128)),
    'null poses': (points, _beside(poses=None)),
    'n 0': (points, _beside(n=0)),
    'n 2^22 + 1': (points, _beside(n=(1 << 22) + 1)),
    'null grid': (spatial, _beside(grid=None)),
    'res 2': (spatial, _beside(res=2)),
    'not progressive': (spatial, _plain),
    'PPE': (spatial, _set(encoding=4, enc_dim=27, k_active=27)),
    'progressive, null mask': (lambda y: flownet(y) and not spatial(y), _set(mask=None)),
    'k_active -1': (lambda y: flownet(y) and not sample(y), _set(k_active=-1)),
    'k_active enc_dim + 1': (lambda y: flownet(y) and not sample(y), _enc_dim_plus_1),
    'null w[1]': (lambda y: not sample(y), _null_w1),
    'saved_bytes 16': (lambda y: not sample(y), _set(saved_bytes=16)),
    'workspace_bytes 16': (lambda y: backward(y) or packs(y), _set(workspace_bytes=16)),
    'workspace at FAKE + 4': (lambda y: backward(y) or packs(y), _set(workspace=FAKE + 4)),
    'progressive forward, null workspace': (packs, _set(workspace=None)),
    'null g_enc_a': (encgrad, _beside(g_enc_a=None)),
    'RBF with ENCGRAD': (lambda y: encgrad(y) or (posegrad(y) and flownet(y)), _rbf_with_encgrad),
    'enc_workspace_bytes 16': (encgrad, _beside(enc_ws_bytes=16)),
    'null g_poses': (posegrad, _beside(g_poses=None)),
    'extra_workspace_bytes 16': (lambda y: posegrad(y) and flownet(y), _beside(extra_ws_bytes=16)),
    'domain_dim 2, T 2': (lambda y: takes_dim(y) and not points(y), _set(T=2)),
    'domain_dim 2, PE': (takes_dim, _set(encoding=4, enc_dim=26, k_active=26)),
    'domain_dim 2, PIECEWISE': (takes_dim, _set(encoding=5)),
    'domain_dim 4': (takes_dim, _beside(dim=4)),
    'omega inf': (siren, _set(omega=math.inf)),
}


def cases():
    return [(symbol, defect) for symbol in OLD for defect, (applies, _) in DEFECTS.items() if applies(symbol)]


def call_descriptor(_lib, s):
    return _lib.FlowNetCall(mode=s.mode, domain_dim=s.dim, poses=s.poses, n=s.n, grid=s.grid, res=s.res, centre_scale=C.cast(s.cs, C.c_void_p),
                            g_enc_a=s.g_enc_a, enc_workspace=s.enc_ws, enc_workspace_bytes=s.enc_ws_bytes, g_poses=s.g_poses,
                            extra_workspace=s.extra_ws, extra_workspace_bytes=s.extra_ws_bytes)


def new_call(_lib, symbol, s):
    """the call `symbol` made, through the entry point that remains: (return code, sininn_last_error())"""
    lib = _lib.lib()
    fn = getattr(lib, OLD[symbol][0])
    a = None if s.args is None else C.byref(s.args)
    tail = (s.out, None) if 'sample_mask' in symbol else (None,)
    rc = fn(a, C.byref(call_descriptor(_lib, s)), *tail)
    return rc, lib.sininn_last_error().decode()


def test_five_entry_points_remain_and_twenty_are_gone():
    from sin_inn_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', '..', 'include', 'sininn.h')).read()
    assert len(REMAIN) == 5 and len(REMOVED) == 20
    for name in REMAIN:
        fn = getattr(lib, name)
        assert name in _lib.EXPORTED and f'int {name}(' in header, name
        assert fn.restype is C.c_int and fn.argtypes[1] is C.POINTER(_lib.FlowNetCall) and fn.argtypes[-1] is C.c_void_p
    for name in REMOVED:
        assert name not in _lib.EXPORTED and not hasattr(lib, name) and name + '(' not in header, name
    assert lib.sininn_version() == 4
    assert lib.sininn_sizeof(7) == C.sizeof(_lib.FlowNetArgs) == 280 and lib.sininn_sizeof(9) == C.sizeof(_lib.SirenArgs) == 280
    assert lib.sininn_sizeof(10) == C.sizeof(_lib.FlowNetCall) and lib.sininn_sizeof(11) == 0


def test_every_recorded_refusal_is_unchanged():
    from sin_inn_amd import _lib
    golden = json.load(open(GOLDEN))
    recorded = {(e['symbol'], e['defect']): e['message'] for e in golden['entries']}
    assert golden['commit'] == 'a1fffaf' and len(recorded) == len(golden['entries'])
    assert set(recorded) == set(cases()) and {s for s, _ in recorded} == set(OLD)
    replayed, wrong = 0, []
    for (symbol, defect), want in recorded.items():
        s = base(_lib, symbol)
        DEFECTS[defect][1](s)
        rc, got = new_call(_lib, symbol, s)
        replayed += 1
        if rc == 0 or got != want:
            wrong.append((symbol, defect, rc, got, want))
    assert not wrong, wrong
    assert replayed == len(golden['entries'])


# what only a call descriptor can get wrong: (entry point, fields of the descriptor, words of the sentence that names the combination)
NEW_REFUSALS = [
    ('sininn_flownet_forward', dict(struct_bytes=8), ('flownet_forward:', 'call descriptor', 'struct_bytes is 8')),
    ('sininn_siren_backward', dict(struct_bytes=8), ('siren_backward:', 'call descriptor', 'struct_bytes is 8')),
    ('sininn_flownet_backward', dict(mode=16 | AT_POINTS), ('flownet_backward_points:', 'unknown mode bits 0x10')),
    ('sininn_flownet_forward', dict(domain_dim=2, mode=SPATIAL), ('flownet_forward_spatial:', 'domain_dim 2 with SPATIAL')),
    ('sininn_flownet_backward', dict(domain_dim=2, mode=ENCGRAD), ('flownet_backward_encgrad:', 'domain_dim 2 with ENCGRAD')),
    ('sininn_flownet_backward', dict(domain_dim=2, mode=AT_POINTS | POSEGRAD), ('flownet_backward_posegrad_points:', 'domain_dim 2 with POSEGRAD')),
    ('sininn_flownet_backward', dict(mode=POSEGRAD), ('flownet_backward_posegrad:', 'POSEGRAD without AT_POINTS')),
    ('sininn_flownet_backward', dict(mode=SPATIAL | POSEGRAD), ('flownet_backward_posegrad_spatial:', 'POSEGRAD without AT_POINTS')),
    ('sininn_flownet_sample_mask', dict(mode=0), ('flownet_sample_mask:', 'sample_mask without SPATIAL')),
    ('sininn_flownet_sample_mask', dict(mode=AT_POINTS), ('flownet_sample_mask_points:', 'sample_mask without SPATIAL')),
    ('sininn_flownet_sample_mask', dict(mode=SPATIAL | ENCGRAD), ('flownet_sample_mask:', 'ENCGRAD / POSEGRAD outside a backward call')),
    ('sininn_flownet_forward', dict(mode=ENCGRAD), ('flownet_forward:', 'ENCGRAD / POSEGRAD outside a backward call')),
    ('sininn_flownet_forward', dict(mode=AT_POINTS | POSEGRAD), ('flownet_forward_points:', 'ENCGRAD / POSEGRAD outside a backward call')),
    ('sininn_siren_forward', dict(mode=SPATIAL), ('siren_forward_spatial:', 'SPATIAL with SIREN')),
    ('sininn_siren_backward', dict(mode=ENCGRAD), ('siren_backward_encgrad:', 'ENCGRAD with SIREN')),
    ('sininn_siren_backward', dict(mode=AT_POINTS, domain_dim=2), ('siren_backward_points:', 'domain_dim 2', 'SIREN')),
    ('sininn_siren_forward', dict(mode=POSEGRAD | AT_POINTS), ('siren_forward_points:', 'ENCGRAD / POSEGRAD outside a backward call')),
    ('sininn_siren_backward', dict(mode=POSEGRAD), ('siren_backward_posegrad:', 'POSEGRAD without AT_POINTS')),
]


@pytest.mark.parametrize('entry,fields,words', NEW_REFUSALS, ids=[f'{w[0]} {w[-1]}' for _, _, w in NEW_REFUSALS])
def test_new_refusals_name_the_combination(entry, fields, words):
    """each comes back non-zero from the validator, before the network descriptor is looked at (it is otherwise a call that nothing else
    refuses, and a null one gives the same sentence), under the name the mode spells"""
    from sin_inn_amd import _lib
    lib = _lib.lib()
    old = next(y for y, (new, mode, _) in OLD.items() if new == entry and ('siren' in y) == ('siren' in entry))
    for null_args in (False, True):
        s = base(_lib, old)
        s.mode, s.dim, s.g_enc_a = 0, 3, FAKE
        call = call_descriptor(_lib, s)
        for k, v in fields.items():
            setattr(call, k, v)
        tail = (FAKE, None) if 'sample_mask' in entry else (None,)
        assert getattr(lib, entry)(None if null_args else C.byref(s.args), C.byref(call), *tail) != 0
        msg = lib.sininn_last_error().decode()
        assert msg.startswith(words[0]) and all(w in msg for w in words), msg


def test_encgrad_beside_posegrad_is_stated_by_its_bit():
    """the old posegrad entry points read a null g_enc_a as "no frequency gradient"; under the bit it is a refusal of its own"""
    from sin_inn_amd import _lib
    s = base(_lib, 'sininn_flownet_backward_posegrad_points')
    s.args.encoding, s.mode, s.g_enc_a = 1, s.mode | ENCGRAD, None
    rc, msg = new_call(_lib, 'sininn_flownet_backward_posegrad_points', s)
    assert rc != 0 and msg == 'flownet_backward_posegrad_points: null g_enc_a'


def test_a_null_call_descriptor_is_the_plain_call():
    """the same refusal, word for word, as an explicit descriptor of mode 0 at three coordinates"""
    from sin_inn_amd import _lib
    lib = _lib.lib()
    for symbol in ('sininn_flownet_forward', 'sininn_flownet_backward', 'sininn_siren_forward', 'sininn_siren_backward'):
        s = base(_lib, symbol)
        s.args.w[1] = None
        rc, want = new_call(_lib, symbol, s)
        assert rc != 0 and 'null weight / bias 1' in want
        assert getattr(lib, symbol)(C.byref(s.args), None, None) != 0 and lib.sininn_last_error().decode() == want
