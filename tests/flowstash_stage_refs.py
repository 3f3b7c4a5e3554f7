"""TEST INFRASTRUCTURE: the error stash (`flowtrainer.error_stash`, csrc/flowtrain.hip) checked stage by stage from the
buffers a call leaves in the caller's workspace (tests/test_flowstash_stages_host.py, tests/test_gpu_flowstash_stages.py).  numpy, and
torch on the CPU for `axis_cells` of tests/flowstash_refs.py; nothing here calls an operator of the package.

    CASES, case(name)            the inputs as fp32 numpy arrays, the starting logs, the properties a case is named for
    workspace(case), split(case, ws)   a NaN-filled workspace with SURPLUS floats to spare; its parts R1, R2, Cy, Cx and the surplus
    stages(case, e, ws, buf, cnt)     every stage of one call, each given the stage before it as the call left it
    model(case, order, defect)        the three kernels one rounding at a time in numpy fp32: the 64-lane xor butterflies, the chunk
                                      skip, the (0 + 1) + (2 + 3) wave combine; two orders; one seeded defect at a time (DEFECTS)

U = 2^-24.  THE SUM BUDGET.  n non-negative fp32 terms added in n - 1 fp32 additions in any order (a tree, a chain, lanes then a
butterfly): every addition is within U of a partial sum that is at most A (1 + U)^(n - 1), A the exact sum of the terms, so the result
is within (n - 1) U A (1 + n U) of A; (n - 1)(1 + n U) <= n while n (n - 1) U <= 1, that is for n <= 4096, whence the budget n U A
(`sum_check` asserts n <= 4096).  A kernel that adds exact zeros between the terms (a lane without a term, a skipped chunk) adds no
rounding: x + 0 is x.  So n = 0 gives an exact 0 and n = 1 the term itself; both are asserted as equalities.  The float64 reference
sum of at most 4096 fp32 terms is itself within 4096 * 2^-53 A of A, 2^-29 of the smallest budget.

    stage 0   E == e32(case): every operation of es_direction and the 0.5 (d1 + d2) restated, one rounding each, ((d0 + d1) + d2) / C
    stage 1   R1[b][y][tile][ix]: the terms fl32(a_x E) of the pixels of the tile whose lower / upper x cell is ix (a pixel clamped
              to one cell with both halves gives two terms), E the call's own, a_x from `axis_cells`: sum budget
    stage 2   R2[b][iy][ix]: row = the fp32 sum of the call's own R1 over the tiles in tile order (bit for bit: the order is the
              kernel's), terms fl32(a_y row): sum budget.  Cy[iy], Cx[ix]: the terms are the axis weights themselves: sum budget
    stage 3   log_buffer == fl32(old + acc), log_counter == fl32(old + fl32(fl32(ct cy) cx)) bit for bit from the call's own R2, Cy,
              Cx: acc and ct are formed by one thread, b in index order, the lower half before the upper, every operation rounded once
Every slot of the workspace must have been written (the NaN fill shows one that was not) and the surplus must still be NaN.
"""
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowstash_refs as S  # noqa: E402  (axis_cells, stash, check_logs: torch expressions, no operator of the package)

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
ES_TX, ES_MAX_RES = 1024, 1024           # csrc/flowtrain.hip: pixels of a row per block; the sentinel of an empty chunk's range
SURPLUS = 7                              # floats a test's workspace is larger than needed by
IDENTITY = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
ORDERS = ('documented', 'reversed')


# ---- cases ------------------------------------------------------------------------------------------------------------------------

# name: B, C, mask channels, H, W, res, kind of times, of ys, of xs, flags ('scaled': centre and scale as set_scale makes them;
# 'fractional': masks in [0, 1), for stages 0 and 1 -- the end-to-end bound of flowstash_refs assumes 0 / 1 masks)
CASES = {
    'w63_res3':           (1, 3, 3, 1, 63, 3, 'asc', 'asc', 'asc', ()),
    'w64_res4_c1':        (1, 1, 1, 3, 64, 4, 'asc', 'asc', 'desc', ()),
    'w65_res5_b5':        (5, 3, 1, 4, 65, 5, 'shuffled', 'asc', 'asc', ()),
    'w1023_res50':        (1, 3, 3, 1, 1023, 50, 'asc', 'asc', 'asc', ()),
    'w1024_res64_ydesc':  (1, 3, 1, 3, 1024, 64, 'asc', 'desc', 'asc', ()),
    'w1025_res65_c1':     (1, 1, 1, 5, 1025, 65, 'asc', 'asc', 'asc', ()),
    'w2048_xshuffled':    (1, 3, 3, 2, 2048, 5, 'asc', 'asc', 'shuffled', ()),
    'w2049_res130':       (1, 3, 1, 3, 2049, 130, 'asc', 'asc', 'asc', ()),
    'h70_yshuffled_b5':   (5, 3, 3, 70, 33, 7, 'shuffled', 'shuffled', 'asc', ()),
    'x_const':            (1, 3, 3, 3, 130, 5, 'asc', 'asc', 'const', ()),
    'x_past':             (1, 3, 1, 4, 200, 4, 'asc', 'asc', 'past', ()),
    'x_edge':             (1, 1, 1, 3, 150, 5, 'asc', 'asc', 'edge', ()),
    'y_const':            (1, 3, 3, 5, 70, 5, 'asc', 'const', 'asc', ()),
    'y_past':             (1, 3, 1, 6, 70, 4, 'asc', 'past', 'asc', ()),
    'y_edge':             (1, 1, 1, 6, 70, 5, 'asc', 'edge', 'asc', ()),
    't_asc':              (5, 3, 3, 3, 65, 5, 'asc', 'asc', 'asc', ()),
    't_desc':             (5, 3, 1, 3, 65, 5, 'desc', 'asc', 'asc', ()),
    't_const':            (5, 1, 1, 3, 65, 5, 'const', 'asc', 'asc', ()),
    't_past':             (5, 3, 3, 3, 65, 4, 'past', 'asc', 'asc', ()),
    't_edge':             (5, 3, 3, 3, 65, 5, 'edge', 'asc', 'asc', ()),
    'scaled':             (5, 3, 3, 6, 70, 7, 'asc', 'asc', 'asc', ('scaled',)),
    'fractional_c3_m3':   (1, 3, 3, 3, 1025, 5, 'asc', 'asc', 'asc', ('fractional',)),
    'fractional_c3_m1':   (5, 3, 1, 3, 65, 5, 'shuffled', 'asc', 'asc', ('fractional',)),
    'fractional_c1':      (1, 1, 1, 4, 130, 65, 'asc', 'asc', 'asc', ('fractional',)),
}
SHUFFLED_TIMES = (0.3, -1.0, 0.3, 1.0, -0.2)     # unsorted, one time twice: two frames in the same two time cells
SCALED_RANGES = ((0.1, 0.9), (-0.8, 1.2), (-2.0, 3.0))


def tiles(w):
    return (w + ES_TX - 1) // ES_TX


def base_trips(res):
    return (res + 63) // 64


def workspace_floats(b, h, w, res):
    """R1, R2, Cy, Cx, in that order (flow_error_stash_launch)"""
    return b * h * tiles(w) * res + b * res * res + 2 * res


def axis32(v, d, res, cs):
    """`axis_cell` of csrc/spatial_cells.h in numpy fp32, one rounding per operation: (i0, i1) int64, (a0, a1) fp32, u"""
    v = np.asarray(v, F32)
    xs = (v - F32(cs[d])) * F32(cs[3 + d])
    u = ((xs + F32(1)) * F32(0.5)) * F32(max(res - 2, 1)) + F32(0.5)
    f0, f1 = np.floor(u), np.ceil(u + F32(1e-6))
    top = F32(res - 1)
    i0 = np.minimum(np.maximum(f0, F32(0)), top).astype(np.int64)
    i1 = np.minimum(np.maximum(f1, F32(0)), top).astype(np.int64)
    return (i0, i1), (f1 - u, u - f0), u


def _v_of_u(u, res):
    """the identity-scaled coordinate whose u is about `u`"""
    return ((np.asarray(u, F64) - 0.5) / max(res - 2, 1) * 2 - 1).astype(F32)


def _edge_coordinate(k, res):
    """a coordinate whose fp32 u lies within 1e-6 below the cell boundary k and whose u + 1e-6 passes it: floor(u) = k - 1,
    ceil(u + 1e-6) = k + 1, the two weights add up to 2.  Found by stepping down from the boundary's coordinate through the floats
    (np.nextafter; a coordinate of 0 is left in steps of 2^-26, the spacing that still moves v + 1)"""
    v = _v_of_u(float(k), res)[()]
    for _ in range(512):
        (_, _), (a0, a1), u = axis32(v, 0, res, IDENTITY)
        if u < k and k - float(u) <= 1e-6 and float(a0) + float(a1) > 1.5:
            return v
        below = np.nextafter(v, F32(-np.inf))
        v = below if abs(float(v)) >= 2.0 ** -20 else F32(float(v) - 2.0 ** -26)
    raise AssertionError((k, res))


def _axis(kind, n, res, rng, times=False):
    if kind == 'asc' or kind == 'desc':
        v = np.linspace(-1, 1, n).astype(F32) if n > 1 else np.array([0.3], F32)
        return v if kind == 'asc' else v[::-1].copy()
    if kind == 'shuffled':
        if times:
            assert n == len(SHUFFLED_TIMES)
            return np.array(SHUFFLED_TIMES, F32)
        return rng.permutation(np.linspace(-1, 1, n).astype(F32))
    if kind == 'const':
        return np.full(n, 0.3, F32)
    if kind == 'past':                                   # u from -1.3 to res + 0.3: both halves in cell 0, then in cell res - 1
        return _v_of_u(np.linspace(-1.3, res + 0.3, n), res)
    if kind == 'edge':
        v = np.linspace(-1, 1, n).astype(F32)
        ks = list(range(1, res - 1))
        at = np.linspace(1, n - 1, len(ks)).astype(int)
        for p, k in zip(at, ks):
            v[p] = _edge_coordinate(k, res)
        return v
    raise KeyError(kind)


def _set_scale(times, ys, xs):
    """centre and scale as StashedSpatialController.set_scale makes them from the points of the grid, in fp32"""
    lo = torch.stack([torch.from_numpy(v).min() for v in (times, ys, xs)])
    hi = torch.stack([torch.from_numpy(v).max() for v in (times, ys, xs)])
    return tuple(float(v) for v in torch.cat(((hi + lo) / 2, 2 / (hi - lo))))


_CASE = {}


def case(name):
    """dict: six (s1, i1, m1, s2, i2, m2), axes (times, ys, xs), res, cs, the extents, old (starting logs, non-zero), flags"""
    if name in _CASE:
        return _CASE[name]
    b, c, cm, h, w, res, tk, yk, xk, flags = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    s1, i1, s2, i2 = (rng.random((b, c, h, w), dtype=F32) for _ in range(4))
    for s in (s1, s2):                                   # splats with exact zeros: pixels nothing was splatted to
        s *= rng.random((b, 1, h, w)) > 0.15
    masks = []
    for s in (s1, s2):
        if 'fractional' in flags:
            m = rng.random((b, cm, h, w), dtype=F32) * (rng.random((b, cm, h, w)) > 0.1)
        else:                                            # 0 / 1, as a step makes them: occlusion times splat != 0
            occl = (rng.random((b, 1, h, w)) > 0.3).astype(F32)
            m = occl * (s != 0) if cm == c else occl * (s != 0).all(1, keepdims=True)
        if h > 2 and w > 2:
            m[:, :, 1, 1] = 0                            # a pixel masked in every channel and both directions
        masks.append(np.ascontiguousarray(m, F32))
    if 'scaled' in flags:
        times, ys, xs = (np.linspace(lo, hi, n).astype(F32) for (lo, hi), n in zip(SCALED_RANGES, (b, h, w)))
        cs = _set_scale(times, ys, xs)
    else:
        times, ys, xs = _axis(tk, b, res, rng, times=True), _axis(yk, h, res, rng), _axis(xk, w, res, rng)
        cs = IDENTITY
    # starting logs that are not 0, and small beside what a call adds: a last-bit difference of acc survives the addition to them
    old = tuple((rng.random(res ** 3, dtype=F32) + F32(1)) * F32(2.0 ** -10) for _ in range(2))
    _CASE[name] = dict(name=name, six=(s1, i1, masks[0], s2, i2, masks[1]), axes=(times, ys, xs), res=res, cs=cs, B=b, C=c, cm=cm, H=h,
                       W=w, old=old, flags=flags, kinds=(tk, yk, xk))
    return _CASE[name]


def cells_of(case, d):
    """((i0, i1) int64, (a0, a1) fp32) numpy, of axis d (0: times, 1: ys, 2: xs), from `axis_cells` of flowstash_refs"""
    (i0, i1), (a0, a1) = S.axis_cells(torch.from_numpy(case['axes'][d]), d, case['res'], case['cs'])
    return (i0.numpy(), i1.numpy()), (a0.numpy(), a1.numpy())


def workspace(case):
    need = workspace_floats(case['B'], case['H'], case['W'], case['res'])
    return np.full(need + SURPLUS, np.nan, F32)


def split(case, ws):
    """views R1 (B, H, tiles, res), R2 (B, res, res) as [b][iy][ix], Cy, Cx, surplus of the flat workspace"""
    b, h, res, nt = case['B'], case['H'], case['res'], tiles(case['W'])
    n1, n2 = b * h * nt * res, b * res * res
    return (ws[:n1].reshape(b, h, nt, res), ws[n1:n1 + n2].reshape(b, res, res), ws[n1 + n2:n1 + n2 + res],
            ws[n1 + n2 + res:n1 + n2 + 2 * res], ws[n1 + n2 + 2 * res:])


# ---- the restatements shared by the checks and the model ---------------------------------------------------------------------------

def e32(case, order='documented', defect=None):
    """E (B, H, W) in fp32, one rounding per operation"""
    b, c, cm, h, w = case['B'], case['C'], case['cm'], case['H'], case['W']
    s1, i1, m1, s2, i2, m2 = case['six']

    def direction(s, i, m):
        d = []
        for ch in range(c):
            if defect == 'mask1 read at channel c' and cm == 1:       # (b cm + c) H W + r with cm = 1: the plane of frame b + c
                mk = m.reshape(-1, h, w)[(np.arange(b) + ch) % b]
            else:
                mk = m[:, 0 if cm == 1 else ch]
            d.append(np.abs(s[:, ch] * mk - i[:, ch] * mk))
        if order == 'reversed':
            d = d[::-1]
        total = d[0]
        for x in d[1:]:
            total = total + x
        return total / F32(3 if defect == '<1> divides by 3' else c)
    e = F32(0.5) * (direction(s1, i1, m1) + direction(s2, i2, m2))
    assert e.dtype == F32
    return e


def frames32(case, r2, cy, cx, order='documented', defect=None):
    """(acc, prod) (res^3,) fp32: what error_frames adds to log_buffer and to log_counter, from R2 [b][iy][ix], Cy, Cx"""
    res = case['res']
    (i0, i1), (a0, a1) = cells_of(case, 0)
    acc, ct = np.zeros((res, res, res), F32), np.zeros(res, F32)          # acc as [ix][iy][it]: cell = it + res (iy + res ix)
    frames = range(case['B']) if order == 'documented' else range(case['B'] - 1, -1, -1)
    for b in frames:
        v = r2[b].T                                                       # [ix][iy]
        halves = ((i0[b], a0[b]), (i1[b], a1[b]))
        for it, a in (halves if order == 'documented' else halves[::-1]):
            acc[:, :, it] = acc[:, :, it] + a * v
            ct[it] = ct[it] + a
    if defect == 'log_counter is ct (cy cx)':
        prod = ct[None, None, :] * (cy[None, :, None] * cx[:, None, None])
    else:
        prod = (ct[None, None, :] * cy[None, :, None]) * cx[:, None, None]
    if defect == 'cell decode ix fastest':                                # thread `cell` takes it = cell / res^2, ix = cell % res
        acc, prod = acc.transpose(2, 1, 0), prod.transpose(2, 1, 0)
    assert acc.dtype == F32 and prod.dtype == F32
    return np.ascontiguousarray(acc).reshape(-1), np.ascontiguousarray(prod).reshape(-1)


# ---- the checks --------------------------------------------------------------------------------------------------------------------

def _bits_differ(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    assert a.shape == b.shape
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def sum_check(got, index, terms, slots):
    """got (slots,) fp32 against the exact sums of the fp32 `terms` by `index`: (worst error / budget over the slots of two and more
    terms, the number of slots that break an equality: n = 0 not an exact 0, n = 1 not the term, a value that is not finite)"""
    terms = np.asarray(terms)
    assert terms.dtype == F32 and bool((terms >= 0).all())
    index, got = np.asarray(index).reshape(-1), np.asarray(got, F32).reshape(-1).astype(F64)
    n = np.bincount(index, minlength=slots)
    a = np.bincount(index, weights=terms.reshape(-1).astype(F64), minlength=slots)
    assert n.size == slots == got.size and int(n.max()) <= 4096
    bad = ~np.isfinite(got)
    err = np.where(bad, np.inf, np.abs(got - a))
    broken = int(bad.sum()) + int(((n <= 1) & ~bad & (got != a)).sum())
    budget = n * U * a
    many = n >= 2
    ratio = np.where(err[many] == 0, 0.0, err[many] / np.maximum(budget[many], 1e-300))
    return (float(ratio.max()) if ratio.size else 0.0), broken


def stage0(case, e, order='documented'):
    return _bits_differ(e, e32(case, order))


def stage1(case, e, r1):
    b, h, w, res, nt = case['B'], case['H'], case['W'], case['res'], tiles(case['W'])
    (i0, i1), (a0, a1) = cells_of(case, 2)
    e = np.asarray(e, F32)
    t0, t1 = a0[None, None, :] * e, a1[None, None, :] * e                 # fl32(a_x E)
    slot = ((np.arange(b)[:, None, None] * h + np.arange(h)[None, :, None]) * nt + (np.arange(w) // ES_TX)[None, None, :]) * res
    return sum_check(r1, np.concatenate([(slot + i0).reshape(-1), (slot + i1).reshape(-1)]),
                     np.concatenate([t0.reshape(-1), t1.reshape(-1)]), b * h * nt * res)


def rows32(r1):
    """the fp32 sum of R1 over the tiles in tile order: (B, H, res)"""
    row = r1[:, :, 0]
    for t in range(1, r1.shape[2]):
        row = row + r1[:, :, t]
    return row


def stage2(case, r1, r2, cy, cx):
    """((ratio, broken) of R2, of Cy, of Cx)"""
    b, h, res = case['B'], case['H'], case['res']
    (i0, i1), (a0, a1) = cells_of(case, 1)
    row = rows32(np.asarray(r1, F32))
    t0, t1 = a0[None, :, None] * row, a1[None, :, None] * row             # fl32(a_y row), (B, H, res)
    ix = np.arange(res)[None, None, :]
    slot = lambda i: ((np.arange(b)[:, None, None] * res + i[None, :, None]) * res + ix).reshape(-1)
    out = [sum_check(r2, np.concatenate([slot(i0), slot(i1)]), np.concatenate([t0.reshape(-1), t1.reshape(-1)]), b * res * res)]
    for d, got in ((1, cy), (2, cx)):
        (j0, j1), (w0, w1) = cells_of(case, d)
        out.append(sum_check(got, np.concatenate([j0, j1]), np.concatenate([w0, w1]), res))
    return tuple(out)


def stage3(case, r2, cy, cx, buf, cnt, order='documented'):
    """(log_buffer values, log_counter values) that differ in bits from old + what frames32 makes of the call's own R2, Cy, Cx"""
    acc, prod = frames32(case, np.asarray(r2, F32), np.asarray(cy, F32), np.asarray(cx, F32), order)
    return _bits_differ(buf, case['old'][0] + acc), _bits_differ(cnt, case['old'][1] + prod)


def stages(case, e, ws, buf, cnt, order='documented'):
    """every stage of one call that started from case['old'] and a workspace of `workspace(case)`"""
    r1, r2, cy, cx, surplus = split(case, np.asarray(ws, F32))
    s2 = stage2(case, r1, r2, cy, cx)
    return dict(stage0=stage0(case, e, order), stage1=stage1(case, e, r1), R2=s2[0], Cy=s2[1], Cx=s2[2],
                stage3=stage3(case, r2, cy, cx, buf, cnt, order),
                unwritten=int(np.isnan(ws[:ws.size - surplus.size]).sum()), surplus_touched=int((~np.isnan(surplus)).sum()))


def failures(r):
    """stage -> failed, of a result of `stages`"""
    two = any(ratio > 1 or broken > 0 for ratio, broken in (r['R2'], r['Cy'], r['Cx']))
    return {'stage 0': r['stage0'] > 0, 'stage 1': r['stage1'][0] > 1 or r['stage1'][1] > 0, 'stage 2': two,
            'stage 3': r['stage3'] != (0, 0), 'fill': r['unwritten'] > 0 or r['surplus_touched'] > 0}


def describe(r):
    return (f"stage 0 {r['stage0']} bits;  stage 1 {r['stage1'][0]:.3f} ({r['stage1'][1]});  stage 2 R2 {r['R2'][0]:.3f} ({r['R2'][1]}) "
            f"Cy {r['Cy'][0]:.3f} ({r['Cy'][1]}) Cx {r['Cx'][0]:.3f} ({r['Cx'][1]});  stage 3 {r['stage3'][0]} + {r['stage3'][1]} bits;  "
            f"unwritten {r['unwritten']}, surplus touched {r['surplus_touched']}")


def end_to_end(case, buf, cnt, e=None, what=''):
    """`check_logs` of flowstash_refs, unchanged, on what one call adds to zeroed logs"""
    six = [torch.from_numpy(a) for a in case['six']]
    axes = [torch.from_numpy(a) for a in case['axes']]
    ref_buf, ref_cnt, n_terms = S.stash(S.error_map(*six), *axes, case['res'], case['cs'])
    assert int(n_terms.sum()) == 8 * case['B'] * case['H'] * case['W']
    S.check_logs(torch.from_numpy(np.ascontiguousarray(buf)), torch.from_numpy(np.ascontiguousarray(cnt)), ref_buf, ref_cnt, n_terms,
                 what=what)


# ---- the model ---------------------------------------------------------------------------------------------------------------------

DEFECTS = (
    'chunk skip tests ix <= clo',
    'upper half compared through c & 0xffff',
    'padding taken as a cell',
    'tile sum starts at tile 1',
    'tile sum stops one short',
    'second base iteration skipped',
    'ix < res guard dropped on the R2 store',
    '<1> divides by 3',
    'mask1 read at channel c',
    'a_y lower and upper swapped',
    'Cx summed over H entries',
    'cell decode ix fastest',
    'clamped pixel counted once',
    'log_counter is ct (cy cx)',
)
_XOR = {'documented': (32, 16, 8, 4, 2, 1), 'reversed': (1, 2, 4, 8, 16, 32)}
_LANES = np.arange(64)


def _butterfly(acc, order):
    """acc (.., 64): the xor butterfly; every lane ends with the same value, lane 0 is returned"""
    for o in _XOR[order]:
        acc = acc + acc[..., _LANES ^ o]
    return acc[..., 0]


def _lanes_sum(contrib, order):
    """contrib (cells, n): lane j adds entries j, j + 64, .. in index order (reversed: from the last), then the butterfly"""
    cells, n = contrib.shape
    pad = (-n) % 64
    chunks = np.concatenate([contrib, np.zeros((cells, pad), F32)], 1).reshape(cells, -1, 64)     # an absent entry adds nothing
    ks = range(chunks.shape[1]) if order == 'documented' else range(chunks.shape[1] - 1, -1, -1)
    acc = np.zeros((cells, 64), F32)
    for k in ks:
        acc = acc + chunks[:, k]
    return _butterfly(acc, order)


def _axis_weight(case, d, n, order):
    (i0, i1), (a0, a1), _ = axis32(case['axes'][d][:n], d, case['res'], case['cs'])
    cell = np.arange(case['res'])[:, None]
    return _lanes_sum(np.where(i0[None] == cell, a0[None], F32(0)) + np.where(i1[None] == cell, a1[None], F32(0)), order)


def model(case, order='documented', defect=None, stats=None):
    """(E, workspace, log_buffer, log_counter, acc, prod) of one call from case['old']: acc and prod are what the call adds, the
    logs of a call on zeroed logs.  `stats` receives chunks_visited / chunks_skipped of error_rows"""
    assert order in ORDERS and (defect is None or defect in DEFECTS)
    b, h, w, res, cs, nt = case['B'], case['H'], case['W'], case['res'], case['cs'], tiles(case['W'])
    ws = workspace(case)
    r1, r2, cy, cx, _ = split(case, ws)
    e = e32(case, order, defect)

    # 1  error_rows: one block per (tile, y, b), one wave per x cell
    (xi0, xi1), (xa0, xa1), _ = axis32(case['axes'][2], 2, res, cs)
    cell = np.arange(res)[:, None]
    visited = skipped = 0
    for tile in range(nt):
        x0 = tile * ES_TX
        n = min(ES_TX, w - x0)
        lo_half, hi_half = np.full(ES_TX, 0xffff), np.full(ES_TX, -1)       # packed = -1: c & 0xffff and c >> 16, neither a cell
        range_lo, range_hi = np.full(ES_TX, ES_MAX_RES), np.full(ES_TX, -1)
        if defect == 'padding taken as a cell':
            lo_half[:], hi_half[:], range_lo[:], range_hi[:] = 0, 0, 0, 0
        lo_half[:n], hi_half[:n] = xi0[x0:x0 + n], xi1[x0:x0 + n]
        range_lo[:n], range_hi[:n] = np.minimum(lo_half[:n], hi_half[:n]), np.maximum(lo_half[:n], hi_half[:n])
        clo, chi = range_lo.reshape(-1, 64).min(1), range_hi.reshape(-1, 64).max(1)
        if defect == 'chunk skip tests ix <= clo':
            visit = ~((cell <= clo[None]) | (cell > chi[None]))
        else:
            visit = ~((cell < clo[None]) | (cell > chi[None]))             # (res, 16)
        eq0 = lo_half[None] == cell
        eq1 = (lo_half[None] == cell) if defect == 'upper half compared through c & 0xffff' else (hi_half[None] == cell)
        visited, skipped = visited + int(visit.sum()) * b * h, skipped + int((~visit).sum()) * b * h
        ks = range(ES_TX // 64) if order == 'documented' else range(ES_TX // 64 - 1, -1, -1)
        for bb in range(b):
            for y in range(h):
                v0, v1 = np.zeros(ES_TX, F32), np.zeros(ES_TX, F32)
                v0[:n], v1[:n] = xa0[x0:x0 + n] * e[bb, y, x0:x0 + n], xa1[x0:x0 + n] * e[bb, y, x0:x0 + n]
                if defect == 'clamped pixel counted once':
                    contrib = np.where(eq0, v0[None], np.where(eq1, v1[None], F32(0)))
                else:
                    contrib = np.where(eq0, v0[None], F32(0)) + np.where(eq1, v1[None], F32(0))
                contrib = contrib.reshape(res, -1, 64)
                acc = np.zeros((res, 64), F32)
                for k in ks:
                    acc = np.where(visit[:, k, None], acc + contrib[:, k], acc)
                r1[bb, y, tile] = _butterfly(acc, order)
    if stats is not None:
        stats.update(chunks_visited=visited, chunks_skipped=skipped)

    # 2  error_columns.  The row of blocks b == B first: the order of blocks is not defined, and this one lets a store past R2 show
    cy[:] = _axis_weight(case, 1, h, order)
    cx[:] = _axis_weight(case, 2, h if defect == 'Cx summed over H entries' else w, order)
    (yi0, yi1), (ya0, ya1), _ = axis32(case['axes'][1], 1, res, cs)
    if defect == 'a_y lower and upper swapped':
        ya0, ya1 = ya1, ya0
    first, last = (1, nt) if defect == 'tile sum starts at tile 1' else (0, nt - 1) if defect == 'tile sum stops one short' else (0, nt)
    n1 = r1.size
    for bb in range(b):
        part = np.zeros((4, res, res), F32)                                # [wave][iy][ix]
        for p in range(4):
            ys_ = list(range(p, h, 4))
            for y in (ys_ if order == 'documented' else ys_[::-1]):
                row = r1[bb, y, first]
                for t in range(first + 1, last):
                    row = row + r1[bb, y, t]
                halves = ((yi0[y], ya0[y]), (yi1[y], ya1[y]))
                for iy, a in (halves if order == 'documented' else halves[::-1]):
                    part[p, iy] = part[p, iy] + a * row
        total = (part[0] + part[1]) + (part[2] + part[3]) if order == 'documented' else (part[3] + part[2]) + (part[1] + part[0])
        if defect == 'second base iteration skipped':
            r2[bb, :, :64] = total[:, :64]
        else:
            r2[bb] = total
        if defect == 'ix < res guard dropped on the R2 store':             # lanes ix = res .. the next multiple of 64 store their 0
            for iy in range(res):
                at = n1 + (bb * res + iy) * res + np.arange(res, base_trips(res) * 64)
                at = at[at < ws.size]                                      # past the workspace: nothing to show it in
                ws[at[at >= n1 + r2.size]] = 0                             # the rows of R2 behind are rewritten by their own blocks

    # 3  error_frames
    acc, prod = frames32(case, r2, cy, cx, order, defect)
    return e, ws, case['old'][0] + acc, case['old'][1] + prod, acc, prod
