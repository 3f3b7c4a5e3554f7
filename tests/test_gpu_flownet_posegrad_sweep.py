"""GPU: the coordinate gradient (flow_at(.., pose_grad=True); flownet_posegrad_kernel<KIND, PROG, SPATIAL> of csrc/flownet.hip, the POSEGRAD
chain kernel of csrc/siren.hip) where tests/test_gpu_flownet_posegrad.py and tests/test_gpu_flownet_spatial_points.py do not take it: past
512 tiles, where a block of the grid-stride loop makes a second trip and reuses its LDS tiles, and under global masks that are open, with
`k_active` at the neighbours of every wave-skip boundary.

Method and budget are the standing ones and are not chosen here: error against the float64 restatement <= MULT = 4 x the unit, the unit the
deviation of the same restatement in fp32 torch from float64, measured in the test; both max-norms relative to max |ref|; the kernel's own
ReLU gates (`saved` > 0) forced in both restatements.  Parameter gradients go through tests/test_gpu_flownet.py's `check` (min(4 x unit,
1e-4)), g_poses through tests/test_gpu_flownet_posegrad.py's (4 x unit), in section B through check_or_zero of
tests/test_gpu_flownet_kactive.py (exact +0 where the float64 reference is identically zero).  g_poses is checked as a whole AND on each
coordinate column alone, relative to that column's own max, with that column's own unit.  g_poses, `saved` and the backward workspaces are NaN before each call, as in the sibling files (run_global: the
posegrad call's extra workspace too).

A. N = 33,123 scattered points (scattered(33123), seed 5): 518 tiles, the last of 35 points; chain_blocks = 512, so blocks 0 .. 5 take the
   tiles 512 .. 517 on a second trip.
  1. float64 parity of g_poses and of every parameter gradient (RFF: g_enc_a of the same call) for one network per instantiation family:
     plain RBF, FFN, RBFG, PE, RFF and siren; global mask PRBF and PFF under prefix_mask(515); SPATIAL PRBF and PRBFG under rand_grid(3)
     at res 3.  RBFG / PRBFG exclude the points rbfg_near_wrap marks from g_poses only, at most 3 % of them (asserted).  One call and
     one pair of references per network, shared by two tests: the output layer's bias has a test of its own.
  2. bitwise (RBF, PRBF global, PRBF SPATIAL, siren): g_poses and the flows of the rows from 32,768 on are those of the list poses[32768:]
     called on its own (355 points, six tiles, one trip per block); two calls at the full N agree; a (33152, 3) buffer whose first N rows
     are passed keeps NaN in the other 29.
B. N = 200 points (three tiles and one of 8), PRBF, PFF, PUFF, PRFF (g_enc_a of the same call too) and PRBFG under prefix_mask(k) for
   k in KS, the neighbours of `256 pass + 64 wave >= k - 3`, and under holes_mask() at k_active = 300; PPE (27 wide, one pass) under
   k in (0, 3, 4, 15, 27).  Per case: g_poses against float64 with that mask in the restatement (k = 0: exact +0); the skipped
   (k_active = k) and the unskipped (k_active = the width) call agree bitwise in flows, g_poses and every gradient; the parameter gradients
   of the posegrad call are bitwise those of the points call without it.  Closed columns of W1 that hold NaN change no bit of g_poses, flows
   or gradients (prefix masks at k in {4, 68, 260} and the holes mask; the global form only: the SPATIAL pack is unmasked by design).

What the file found.  (1) Under holes_mask(), which closes the coordinate y, NaN in the closed columns of W1 came out as NaN in
g_poses[:, y], for all five networks: flownet_posegrad_pack_kernel copied the three coordinate columns of W1 unmasked ("their mask multiplies
the finished sum"), and 0 x (a sum over a NaN column) is NaN.  The pack now writes an exact zero for a coordinate whose global mask is zero,
as the forward pack always did; no other bit of g_poses moves (m_d csum was +-0 before and is +0 now, added to a sum that started at +0).
(2) The output layer's bias gb4 (SIREN gb5) = scale * sum_p up[:, p] stood at 1.82 of its budget at N = 33,123 (and at 0.90 - 0.96 in
the sibling files): a sum of signed terms that largely cancel, added in fp32 in a fixed order.  The chain kernels and the reduce kernels
now add it, and the reduce kernel every bias, in double, rounded once per block and once at the end: 0.163 here, at most 0.31 in the suite.

Measured on an MI355X (`ratio(...)` lines of a run with -s: error / budget, [error, fp32-torch unit]); the tables are in DESIGN 14.8 and 14.9.
  A, g_poses at N = 33,123, the worst of whole / column t / y / x:  RBF 0.378 (x) [4.33e-07, 2.86e-07]  FFN 0.114 (x)  RBFG 0.255 (y)
    PE 0.252 (x)  RFF 0.114 (t)  siren 0.261 (y)  PRBF global 0.3 (t) [6.37e-07, 5.31e-07]  PFF global 0.139 (t)
    PRBF SPATIAL 0.305 (x) [4.52e-07, 3.71e-07]  PRBFG SPATIAL 0.249 (x).
  A, parameter gradients but the output bias, the worst per network: 0.191 (PRBF SPATIAL gb3) .. 0.356 (PE gb1 [3.83e-07, 2.69e-07]);
    g_enc_a of RFF's same call 0.105.  Nothing stands above 0.5.
  A, the output bias (gb4, SIREN gb5): 0.163 [3.46e-08, 5.31e-08] in all ten cases (1.82 [3.86e-07, 5.31e-08] before it was summed in double).
  A, excluded from g_poses: RBFG 557 of 33,123 points (1.7 %), PRBFG 507 of 33,123 (1.5 %); the condition is at most 3 %.
  B, g_poses at N = 200, the worst over all masks and of whole / columns:  PRBF 0.289 (x, holes)  PFF 0.251 (y, k = 67)
    PUFF 0.249 (y, k = 131)  PRFF 0.27 (y, k = 4), g_enc_a 0.192 (k = 67)  PRBFG 0.31 (y, k = 67) [5.35e-07, 4.31e-07]
    PPE 0.294 (x, k = 4).  PRBFG: 0 of 200 points within 1e-6 of a wrap.  26 quantities took the exact branch of check_or_zero
    (k = 0: g_poses and its three columns, six networks; PRFF g_enc_a at k = 0 and k = 3).
  148 tests, 5 s.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_points_refs import restate_points, siren_restate_points  # noqa: E402
from flownet_posegrad_refs import check_whole_and_columns, rbfg_near_wrap, reference_all_grads  # noqa: E402
from flownet_refs import nan_buffers, net_tensors  # noqa: E402
from flownet_spatial_refs import interp_mask  # noqa: E402
from flownet_spatial_refs import restate_points as restate_points_per_point_mask  # noqa: E402
from siren_refs import siren_tensors  # noqa: E402
from test_gpu_flownet import CEIL, F64, MULT, SCALE  # noqa: E402
from test_gpu_flownet import check as check_params  # noqa: E402
from test_gpu_flownet_kactive import K_HOLES, check_or_zero, holes_mask, prefix_mask  # noqa: E402
from test_gpu_flownet_points import Case, scattered  # noqa: E402
from test_gpu_flownet_posegrad import check as check_unit  # noqa: E402
from test_gpu_flownet_posegrad import posegrad, upstream  # noqa: E402
from test_gpu_flownet_spatial_points import NETS as SPATIAL_SEEDS  # noqa: E402
from test_gpu_flownet_spatial_points import GNAMES, Net, rand_grid, run_points  # noqa: E402

assert (MULT, CEIL) == (4.0, 1e-4)                     # the standing budget; this file does not choose one
F32 = torch.float32
NAN = float('nan')
N, SPLIT, NPAD = 33123, 32768, 33152                   # 518 tiles; the second trip starts at tile 512; the list padded to whole tiles
assert (N + 63) // 64 == 518 and N - 517 * 64 == 35 and SPLIT == 512 * 64 and NPAD == 518 * 64 and N - SPLIT == 5 * 64 + 35
PLAIN = ('RBF', 'FFN', 'RBFG', 'PE', 'RFF', 'siren')
BIT_FORMS = ('RBF', 'PRBF global', 'PRBF spatial', 'siren')
NB = 200
KS = (0, 3, 4, 67, 68, 131, 132, 195, 196, 259, 260, 323, 324, 387, 388, 451, 452, 515)
KS_PPE = (0, 3, 4, 15, 27)
B_NETS = ('PRBF', 'PFF', 'PUFF', 'PRFF', 'PRBFG')
B_CASES = [(name, k) for name in B_NETS for k in KS + ('holes',)] + [('PPE', k) for k in KS_PPE]
OWN_SEEDS = {'PUFF': 606, 'PPE': 909}                  # the two progressive networks tests/test_gpu_flownet_spatial_points.py does not build
A1_FORMS = ([('plain', name) for name in PLAIN] + [('global', 'PRBF'), ('global', 'PFF')]
            + [('spatial', 'PRBF'), ('spatial', 'PRBFG')])
_cases, _progs, _past = {}, {}, {}


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


class Prog(Net):
    """`Net` of tests/test_gpu_flownet_spatial_points.py for every progressive network: PUFF and PPE, which that file does not build, get
    seeds of their own; `width` is the mask's length (515; PPE: 27)"""

    def __init__(self, name, dev):
        if name in SPATIAL_SEEDS:
            super().__init__(name, dev)
        else:
            from sin_inn_amd import flownet
            torch.manual_seed(OWN_SEEDS[name])
            self.name, self.dev = name, dev
            self.net = flownet.all_model_dict[name](flownet.ModelParams()).to(dev)
            self.fourier, self.enc_a = False, None
            self.bufs, self.weights = net_tensors(self.net, dev)
            self.names = list(GNAMES)
        self.width = self.net.encoding_dim


def prog(name, dev):
    if name not in _progs:
        _progs[name] = Prog(name, dev)
    return _progs[name]


def case(name, dev):
    if name not in _cases:
        _cases[name] = Case(name, dev)
    return _cases[name]


def prefix_mask_ppe(k):
    """prefix_mask at PPE's width of 27"""
    from sin_inn_amd import flownet
    mask = torch.zeros(27)
    mask[:k] = 1.0
    mask[k - min(3, k):k] = 0.5
    assert flownet.last_open(mask) == k
    return mask


def mask_of(name, key):
    """(host mask, k_active) of a case of section B"""
    if key == 'holes':
        return holes_mask(), K_HOLES
    return (prefix_mask_ppe(key) if name == 'PPE' else prefix_mask(key)), key


def nan_pose_workspace(c, enc_grad):
    """the extra workspace of the posegrad call (the packed W1, then the frequency gradient's workspace), all NaN"""
    from sin_inn_amd import _lib
    a = _lib.FlowNetArgs()
    a.encoding = c.net.encode.kind
    nbytes = _lib.lib().sininn_flownet_posegrad_workspace_bytes(a, int(enc_grad))
    assert nbytes > 0
    return torch.full((nbytes // 4,), NAN, device=c.dev)


def run_global(c, poses, up, hmask, k, pose_grad=True, g_poses=None):
    """forward and backward of a Prog at a pose list under the global mask `hmask` with k_active = k, every buffer NaN before:
    dict(flows, saved, grads (list, g_enc_a last), g_poses)"""
    from sin_inn_amd import flownet
    n = poses.shape[0]
    kw = dict(mask=hmask.to(c.dev), k_active=k, enc_a=c.enc_a)
    saved, ws, ews = nan_buffers(n, c.dev)
    flows, saved = flownet.flownet_forward_points(c.net, poses, SCALE, True, saved, **kw)
    gp = None
    if pose_grad:
        gp = torch.full((n, 3), NAN, device=c.dev) if g_poses is None else g_poses
        out, got = flownet.flownet_backward_points(c.net, poses, SCALE, up, saved, ws, enc_grad=c.fourier, pose_grad=True,
                                                   pose_workspace=nan_pose_workspace(c, c.fourier), g_poses=gp, **kw)
        assert got is gp
    else:
        out = flownet.flownet_backward_points(c.net, poses, SCALE, up, saved, ws, enc_grad=c.fourier,
                                              enc_workspace=ews if c.fourier else None, **kw)
    grads = list(out[0]) + [out[1]] if c.fourier else list(out)
    return dict(flows=flows, saved=saved, grads=grads, g_poses=gp)


def global_reference(c, poses, up, mask, saved):
    """reference_all_grads of a Prog under the global mask, the gates those of `saved`"""
    n = poses.shape[0]
    gates = [saved[l, :n] > 0 for l in range(3)]
    return reference_all_grads(lambda w, e, x, dt: restate_points(c.name, c.bufs if e is None else e, w, x, SCALE, dt, mask, gates),
                               c.weights, poses, up, c.enc_a)


def keep_away_from_wraps(name, bufs, poses):
    """the rows of g_poses that are compared: all (None), or (RBFG / PRBFG) those rbfg_near_wrap does not mark, at most 3 % marked"""
    if name not in ('RBFG', 'PRBFG'):
        return None
    near, n = rbfg_near_wrap(bufs, poses), poses.shape[0]
    print(f'{name}: {int(near.sum())} of {n} points within 1e-6 of a wrap, excluded from g_poses')
    assert int(near.sum()) <= 0.03 * n
    return ~near


def last_bias(names):
    """the bias of the output layer: gb4, SIREN gb5"""
    return max(nm for nm in names if nm.startswith('gb'))


# ---- A1: float64 parity past 512 tiles ----
def past_512_tiles(form, dev):
    """one posegrad call of an A1_FORMS entry at the N points and reference_all_grads of the same call, computed once and shared:
    dict(tag, names, grads (list, g_enc_a last), g_poses, ref, keep)"""
    if form in _past:
        return _past[form]
    kind, name = form
    poses, up = scattered(N, dev), upstream(N, dev)
    if kind == 'plain':
        c = case(name, dev)
        grads, g_poses, saved = posegrad(c, poses, up)
        names, enc, keep = c.names(), None, None
        if c.siren:
            weights = siren_tensors(c.net, dev)
            flows_of = lambda w, e, x, dt: siren_restate_points(w, x, SCALE, dt)  # noqa: E731
        else:
            bufs, weights = net_tensors(c.net, dev)
            keep = keep_away_from_wraps(name, bufs, poses)
            enc = c.kw['enc_a'] if c.learnable else None           # the fp32 matrix the kernels receive
            gates = [saved[l, :N] > 0 for l in range(3)]
            flows_of = lambda w, e, x, dt: restate_points(name, bufs if e is None else e, w, x, SCALE, dt, None, gates)  # noqa: E731
        ref = reference_all_grads(flows_of, weights, poses, up, enc)
    elif kind == 'global':
        c, hmask = prog(name, dev), prefix_mask(515)
        got = run_global(c, poses, up, hmask, 515)
        names, grads, g_poses, keep = c.names, got['grads'], got['g_poses'], None
        ref = global_reference(c, poses, up, hmask.to(dev), got['saved'])
    else:
        c, grid = prog(name, dev), rand_grid(3, dev)
        got = run_points(c, poses, up, grid, 3, scale=SCALE)
        names, grads, g_poses, keep = c.names, got['grads'], got['g_poses'], keep_away_from_wraps(name, c.bufs, poses)
        m64 = interp_mask(grid, 3, poses, F64)                       # a constant of both restatements, from the fp32 cells
        gates = [got['saved'][l, :N] > 0 for l in range(3)]
        ref = reference_all_grads(lambda w, e, x, dt: restate_points_per_point_mask(name, c.bufs, w, x, dt, m64.to(dt), gates).t() * SCALE,
                                  c.weights, poses, up)
    assert len(grads) == len(names) == len(ref[F64]) - 1
    _past[form] = dict(tag=f'{name} {kind} N={N}', names=names, grads=grads, g_poses=g_poses, ref=ref, keep=keep)
    return _past[form]


@pytest.mark.parametrize('kind,name', A1_FORMS)
def test_past_512_tiles_against_float64(dev, kind, name):
    """g_poses, whole and per coordinate column, and every parameter gradient (RFF: g_enc_a) but the output layer's bias, which has
    the next test to itself"""
    r = past_512_tiles((kind, name), dev)
    assert r['g_poses'].shape == (N, 3) and bool(torch.isfinite(r['g_poses']).all())
    check_whole_and_columns(check_unit, f"{r['tag']} g_poses", r['g_poses'], r['ref'][F64][-1], r['ref'][F32][-1], r['keep'])
    for nm, g, r64, r32 in zip(r['names'], r['grads'], r['ref'][F64], r['ref'][F32]):
        assert bool(torch.isfinite(g).all()), nm
        if nm != last_bias(r['names']):
            check_params(f"{r['tag']} {nm}", g, r64, r32)


@pytest.mark.parametrize('kind,name', A1_FORMS)
def test_past_512_tiles_output_bias_against_float64(dev, kind, name):
    """gb4 (SIREN: gb5) = scale * sum_p up[:, p] of the same call.  It does not depend on the network, the mask or the poses: the ten
    cases hold the same four numbers against the same reference, and stand or fall together.

    This test missed its budget when it was written: 1.82 [err 3.86e-07, fp32-torch unit 5.31e-08, budget 2.12e-07].  The unit is
    the deviation of ONE fp32 torch sum of 33,123 terms per channel from float64, below half an ulp here; the chain kernels added the
    same products in fp32 (64 points of a tile in sequence, a block's tiles, then the reduce kernel over the 512 block sums in index
    order), and a numpy restatement of that order in fp32 gave 3.8558003653880995e-07, the kernels' error to the last digit.  The
    kernels now keep this one sum in double (four lanes of a block, and the bias entries of flownet_reduce_kernel / gb5 of
    siren_reduce_kernel) and round once per block and once at the end: 0.163 [err 3.46e-08], the rounding of the result itself"""
    r = past_512_tiles((kind, name), dev)
    i = r['names'].index(last_bias(r['names']))
    check_params(f"{r['tag']} {r['names'][i]}", r['grads'][i], r['ref'][F64][i], r['ref'][F32][i])


# ---- A2: bitwise, the second trip against a first trip ----
def run_form(form, dev, poses, up, g_poses=None):
    """(flows (4, n), g_poses (n, 3)) of one forward and one posegrad call of a BIT_FORMS entry, every buffer NaN before;
    `g_poses`: the tensor that receives the gradient"""
    from sin_inn_amd import flownet
    n = poses.shape[0]
    if form == 'PRBF global':
        out = run_global(prog('PRBF', dev), poses, up, prefix_mask(515), 515, g_poses=g_poses)
        return out['flows'], out['g_poses']
    if form == 'PRBF spatial':
        c, grid = prog('PRBF', dev), rand_grid(3, dev)
        if g_poses is None:
            out = run_points(c, poses, up, grid, 3, scale=SCALE)
            return out['flows'], out['g_poses']
        saved, ws, _ = nan_buffers(n, dev)
        flows, saved = flownet.flownet_forward_spatial_points(c.net, poses, SCALE, True, grid, 3, saved=saved)
        flownet.flownet_backward_spatial_points(c.net, poses, SCALE, up, saved, grid, 3, workspace=ws, pose_grad=True, g_poses=g_poses)
        return flows, g_poses
    c = case(form, dev)
    if g_poses is None:
        flows, _ = c.forward_points(poses, train=False)
        return flows, posegrad(c, poses, up)[1]
    saved, ws = c.nan(n)[:2]
    flows, saved = c.forward_points(poses, saved)
    backward = flownet.siren_backward_points if c.siren else flownet.flownet_backward_points
    backward(c.net, poses, SCALE, up, saved, ws, pose_grad=True, g_poses=g_poses)
    return flows, g_poses


@pytest.mark.parametrize('form', BIT_FORMS)
def test_the_second_trip_gives_the_bits_of_a_first_trip(dev, form):
    """a point's gradient depends on nothing but the point: rows 32768 .. of the full list are tiles 512 .. 517, the second trip of
    blocks 0 .. 5; the same points as a list of their own are tiles 0 .. 5, one trip each"""
    poses, up = scattered(N, dev), upstream(N, dev)
    flows, g = run_form(form, dev, poses, up)
    flows_again, g_again = run_form(form, dev, poses, up)
    assert g.shape == (N, 3) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(flows).all())
    assert torch.equal(g, g_again) and torch.equal(flows, flows_again), 'two calls differ'
    tail_flows, tail_g = run_form(form, dev, poses[SPLIT:].contiguous(), up[:, SPLIT:].contiguous())
    assert tail_g.shape == (N - SPLIT, 3) and bool((tail_g != 0).any())
    differ = (g[SPLIT:] != tail_g).any(1)
    assert not bool(differ.any()), f'g_poses of the second trip differs at {int(differ.sum())} of {N - SPLIT} points'
    assert torch.equal(flows[:, SPLIT:], tail_flows), 'flows'


@pytest.mark.parametrize('form', BIT_FORMS)
def test_rows_beyond_n_of_a_tile_padded_buffer_stay_nan(dev, form):
    """rows p >= N are not written: the last tile holds 35 points, the buffer 29 rows more"""
    poses, up = scattered(N, dev), upstream(N, dev)
    buf = torch.full((NPAD, 3), NAN, device=dev)
    head = buf[:N]
    assert head.is_contiguous() and head.data_ptr() == buf.data_ptr()
    _, got = run_form(form, dev, poses, up, g_poses=head)
    assert got is head and bool(torch.isfinite(buf[:N]).all())
    assert bool(torch.isnan(buf[N:]).all()), 'a row beyond N was written'
    assert torch.equal(buf[:N], run_form(form, dev, poses, up)[1])


# ---- B: open global masks, every wave-skip boundary ----
@pytest.mark.parametrize('name,key', B_CASES)
def test_open_global_mask(dev, name, key):
    c = prog(name, dev)
    hmask, k = mask_of(name, key)
    assert hmask.numel() == c.width
    poses, up = scattered(NB, dev), upstream(NB, dev)
    tag = f'{name} k={key}'
    skip = run_global(c, poses, up, hmask, k)
    full = run_global(c, poses, up, hmask, c.width)
    plain = run_global(c, poses, up, hmask, k, pose_grad=False)
    assert bool(torch.isfinite(skip['g_poses']).all())
    assert torch.equal(skip['flows'], full['flows']) and torch.equal(skip['flows'], plain['flows'])
    assert torch.equal(skip['g_poses'], full['g_poses']), f'{tag}: the skipped and the unskipped path differ in g_poses'
    assert len(skip['grads']) == len(full['grads']) == len(plain['grads']) == len(c.names)
    for nm, a, b, d in zip(c.names, skip['grads'], full['grads'], plain['grads']):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f'{tag} {nm}: the skipped and the unskipped path differ'
        assert torch.equal(a, d), f'{tag} {nm}: the posegrad call and the call without it differ'
    ref = global_reference(c, poses, up, hmask.to(dev), skip['saved'])
    keep = keep_away_from_wraps(name, c.bufs, poses)
    check_whole_and_columns(check_or_zero, f'{tag} g_poses', skip['g_poses'], ref[F64][-1], ref[F32][-1], keep)
    if c.fourier:
        check_or_zero(f'{tag} g_enc_a (same call)', skip['grads'][-1], ref[F64][-2], ref[F32][-2])


@pytest.mark.parametrize('key', (4, 68, 260, 'holes'))
@pytest.mark.parametrize('name', B_NETS)
def test_closed_columns_of_w1_that_hold_nan_change_no_bit(dev, name, key):
    """NaN in W1[:, mask == 0] of the network the kernels read: the `m == 0 ? 0` of flownet_posegrad_pack_kernel (and of the forward and
    encgrad packs) keeps it out of g_poses, the flows and every gradient.  No float64 reference on these weights (0 x NaN is NaN in torch)"""
    c = Prog(name, dev)                                             # a network of its own: its W1 is overwritten
    hmask, k = mask_of(name, key)
    poses, up = scattered(NB, dev), upstream(NB, dev)
    clean = run_global(c, poses, up, hmask, k)
    w1 = c.net.linears()[0].weight
    with torch.no_grad():
        w1[:, (hmask == 0).to(dev)] = NAN
    assert int(torch.isnan(w1).sum()) == 256 * int((hmask == 0).sum()) > 0
    bad = run_global(c, poses, up, hmask, k)
    assert bool(torch.isfinite(clean['g_poses']).all()) and bool((clean['g_poses'] != 0).any())
    assert torch.equal(clean['g_poses'], bad['g_poses']), 'g_poses'
    assert torch.equal(clean['flows'], bad['flows']), 'flows'
    for nm, a, b in zip(c.names, clean['grads'], bad['grads']):
        assert torch.equal(a, b), nm
