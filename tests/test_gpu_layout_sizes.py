"""GPU: the layout, sampler and coupling-tail kernels (csrc/hbm_fast.hip and the part of csrc/elementwise.hip that
tests/test_gpu_elementwise_sizes.py leaves out) past ONE sweep of their grid-stride loops.

The stand-alone tests of these kernels (tests/test_gpu_kernels.py, test_gpu_e2e.py::test_frames_to_u8_modes_bit_exact, tests/test_gpu_irn.py)
run 2x3x16x24 .. 3x32x48x3: a handful of blocks, no block cap binds, no thread makes a second trip, squeeze_rows stops at level 2.
Here every kernel runs past its cap (4096 / 8192 / 16384 blocks of 256 threads) with a partial last trip, with a 1 .. 15 element
tail where the kernel has a vector body, and with a wave that straddles the branch where the kernel has one.

Method (that of tests/test_gpu_elementwise_sizes.py):
  * the reference is plain torch on the GPU (indexing, permute, reshape, integer ops; float64 for the float kernels; the numpy /
    scipy float64 oracle on the CPU for the Bayer kernels) of the same operation; it never calls the kernel under test.  The
    u8 -> float conversion x / 255.f is compared with a 256-entry table divided on the CPU: torch's GPU division by a Python
    scalar multiplies by the reciprocal and is one ulp off a true division for some bytes;
  * every case recomputes the launch plan from the kernel's own formulas, prints it (run with -s) and asserts the property the
    shape exists for;
  * every output buffer is filled with NaN (uint8 outputs: with two different sentinel bytes, one run each) and followed by a guard
    region; gap columns of strided rows and the guard must keep their bits; two calls must agree bit for bit;
  * A (frames_to_u8, squeeze_rows / squeeze, permute_channels, haar, sample_windows, sample_pairs), C's direct packs and D (bayer_bin,
    bayer_demosaic) are EQUAL to the reference, no element excluded, no tolerance;
  * B (coupling_bwd, irn_tail, irn_coupling_bwd) and C's Winograd packs are held per element to a budget derived next to the
    reference: (roundings on the path) x U x the magnitudes of the terms, U = 2^-24, plus the sensitivity of the result to exp /
    atan times the error of the device's expf / atanf.  That library error was measured once on an MI355X as the worst relative
    error of fp32 torch.exp / torch.atan against float64 (2^26 uniform draws per range, a 2^26-point grid, 3 * randn):
        expf  1.4059 U relative = 0.86 ulp (at x = 1.42958; 1.3972 U on [-16, 16] and [-24, 24], worst at x = 9.7473)
        atanf 3.0806 U relative = 2.09 ulp on [-8, 8] and [-64, 64] (at x = -1.56768; 1.5926 U = 0.93 ulp on [-1, 1])
    (1 U relative is between half an ulp and one ulp of the result.)  The allowances below are TWICE the measured figures:
    EXPF_U = 2.82, ATANF_U = 6.17.  `test_device_exp_and_atan_error` prints the figures again and holds them to the allowance.

Worst error / budget measured on an MI355X (`ratio(...)` lines; the same figures are in the table of DESIGN 4):
    haar against float64                 analysis 0.90, synthesis 0.89 (and bitwise equal to the fp32 restatement)
    coupling_bwd                         ds 0.44 (0.43 where |s| > clamp), dt 0.54 (forward: exact), dv 0.54
    irn_tail                             forward 0.985, inverse 0.51
    irn_coupling_bwd                     dv 0.49, dG 0.49 (forward: exact), dh 0.75 (0.75 where the sigmoid saturates)
    Winograd packs                       u_fwd 0.18, u_dgrad 0.15
A ratio close to 1 is expected where ONE rounding is most of the budget: irn_tail's forward ends in v e + g, whose rounding alone
may reach U |out| where |g| >> |v e|, and some of 1.3e7 elements sit just above a power of two (the sibling file's Adam test
reports the same).  64 tests, 4.3 s."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from test_gpu_elementwise_sizes import F64, U, gen, ratio  # noqa: E402

BF = torch.bfloat16
EXPF_U = 2.82         # allowance for the device expf, relative, in U: twice the 1.4059 U measured (docstring)
ATANF_U = 6.17        # allowance for the device atanf: twice 3.0806 U
SECOND = 1.0 + 2.0 ** -10      # the budgets are first-order in U; this covers the products of two error terms


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def O():
    from oracle import sininn_oracle
    return sininn_oracle


# =================================================================================================================================
# plans, buffers
# =================================================================================================================================
def plan(name, total, cap, per_thread=1, threads=256):
    """the launch every kernel here computes: blocks = min(ceil(total / 256), cap), a grid-stride loop over `total` work items"""
    blocks = max(1, min(-(-total // threads), cap))
    sweep = blocks * threads
    p = dict(total=total, blocks=blocks, trips=-(-total // sweep), remainder=total % sweep, per_thread=per_thread)
    print(f'plan({name}) = {p}')
    return p


def past_cap(p, cap):
    """more than one sweep at the block cap, and a partial last trip"""
    return p['blocks'] == cap and p['trips'] >= 2 and p['remainder'] != 0


def same_bits(a, b):
    it = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def untouched(t, fill=float('nan')):
    return same_bits(t, torch.full_like(t, fill))


GUARD = 4096


class Buf:
    """a (B,C,H,W)-shaped view `t` of a flat buffer that is filled with `fill` and followed by a guard region:
    'nchw' contiguous, 'pm' dense pixel-major, 'pmpad' pixel-major rows of C + pad floats (the last `pad` of each row a gap)"""

    def __init__(self, shape, layout, dev, fill=float('nan'), pad=5, dtype=torch.float32, lead=0):
        b, c, h, w = shape
        cs = c + (pad if layout == 'pmpad' else 0)
        n = b * h * w * cs
        self.flat = torch.full((lead + n + GUARD,), fill, device=dev, dtype=dtype)
        body = self.flat[lead:lead + n]
        self.fill, self.guard, self.gap, self.head = fill, self.flat[lead + n:], None, self.flat[:lead]
        if layout == 'nchw':
            self.t = body.view(b, c, h, w)
        else:
            rows = body.view(b, h, w, cs)
            self.t = rows[..., :c].permute(0, 3, 1, 2)
            if cs > c:
                self.gap = rows[..., c:]

    def put(self, values):
        self.t.copy_(values)
        return self

    def clean(self):
        """gap columns, the guard region and the floats before the tensor still hold the fill"""
        return untouched(self.guard, self.fill) and untouched(self.head, self.fill) and \
            (self.gap is None or untouched(self.gap, self.fill))


def dense_pm(t):
    b, c, h, w = t.shape
    return t.stride() == (h * w * c, 1, w * c, c)


# =================================================================================================================================
# A1. frames_to_u8
# =================================================================================================================================
def u8_ref(x, wrap):
    """(B,C,H,W) float -> (B,H,W,C) uint8: clamp(x, 0, 1) * 255 truncated, or the low byte of (int)(x * 255)"""
    if wrap:
        v = ((x * 255.0).to(torch.int32) & 255).to(torch.uint8)
    else:
        v = (x.clamp(0, 1) * 255.0).to(torch.uint8)
    return v.permute(0, 2, 3, 1).contiguous()


def run_frames(x, wrap):
    """sininn_frames_to_u8 into sentinel-filled buffers (two sentinels, one call each) followed by a guard"""
    from sin_inn_amd import _lib, ops
    b, c, h, w = x.shape
    n = x.numel()
    outs = []
    for sentinel in (0xA5, 0x5A):
        buf = torch.full((n + GUARD,), sentinel, device=x.device, dtype=torch.uint8)
        _lib.check(_lib.lib().sininn_frames_to_u8(ops.ptr(x), ops.strides4(x), buf.data_ptr(), b, c, h, w, 1 if wrap else 0, ops._stream()))
        assert bool((buf[n:] == sentinel).all()), 'frames_to_u8 wrote past B*H*W*C bytes'
        outs.append(buf[:n].view(b, h, w, c))
    assert torch.equal(outs[0], outs[1]), 'an output byte kept its sentinel, or two calls differ'
    return outs[0]


def frames_path(x):
    b, c, h, w = x.shape
    return 'dense' if dense_pm(x) and x.data_ptr() % 16 == 0 else 'strided'


def frame_values(shape, dev, seed):
    """[-1, 2) with the values where the conversion turns planted at both ends (the tail of the dense kernel is at the end)"""
    x = torch.rand(shape, device=dev, generator=gen(seed)) * 3 - 1
    special = torch.tensor([0.0, -0.0, 1.0, 1.0 - 2.0 ** -24, 254.0 / 255, 255.0 / 255, 1.0 / 255, 0.999 / 255, -1.0, 1.9999999, 128.0 / 255],
                           device=dev)
    flat = x.permute(0, 2, 3, 1).reshape(-1)
    k = min(special.numel(), flat.numel())
    flat = flat.clone()
    flat[:k] = special[:k]
    flat[flat.numel() - k:] = special[:k]
    b, c, h, w = shape
    return flat.view(b, h, w, c).permute(0, 3, 1, 2)                  # dense pixel-major


@pytest.mark.parametrize('wrap', [False, True], ids=['clamp', 'wrap'])
def test_frames_to_u8_dense_past_one_sweep_with_tail(dev, wrap):
    from sin_inn_amd.functional import frames_to_u8
    shape = (1, 3, 2365, 2365)
    n = 3 * 2365 * 2365
    p = plan('frames_to_u8 dense', n // 16, 4096)
    assert past_cap(p, 4096) and 1 <= n % 16 <= 15, (p, n % 16)
    x = frame_values(shape, dev, 1)
    assert frames_path(x) == 'dense' and float(x.min()) >= -1 and float(x.max()) < 2
    want = u8_ref(x, wrap)
    got = run_frames(x, wrap)
    assert torch.equal(got, want)
    assert torch.equal(frames_to_u8(x, wrap=wrap), want)          # the front end
    if wrap:
        assert bool((x < 0).any()) and bool((x > 1).any()) and int(want.max()) == 255 and int(want.min()) == 0


@pytest.mark.parametrize('wrap', [False, True], ids=['clamp', 'wrap'])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 4111])
def test_frames_to_u8_dense_tail_sizes(dev, n, wrap):
    """tail only (1, 15), no tail (16), one vector + 1 (17), one full block of vectors + 15 (4111)"""
    shape = (1, 3, 1, 5) if n == 15 else (1, 1, 1, n)
    p = plan(f'frames_to_u8 dense n={n}', n // 16, 4096)
    print(f'  vectors {n // 16}, tail {n % 16}')
    x = frame_values(shape, dev, 2 + n)
    assert x.numel() == n and frames_path(x) == 'dense'
    assert torch.equal(run_frames(x, wrap), u8_ref(x, wrap))


@pytest.mark.parametrize('wrap', [False, True], ids=['clamp', 'wrap'])
def test_frames_to_u8_strided_past_one_sweep_and_misaligned_dense(dev, wrap):
    """NCHW input: the strided kernel past 8192 blocks.  The same values pixel-major but 4 bytes off 16-byte alignment must take
    the strided kernel too; pixel-major and aligned they take the dense one.  All three give the same bytes."""
    shape = (3, 3, 513, 511)
    n = 3 * 3 * 513 * 511
    p = plan('frames_to_u8 strided', n, 8192)
    assert past_cap(p, 8192), p
    xd = frame_values(shape, dev, 3)
    xn = xd.contiguous()
    off = Buf(shape, 'pm', dev, lead=1).put(xd).t
    assert frames_path(xn) == 'strided' and frames_path(xd) == 'dense'
    assert dense_pm(off) and off.data_ptr() % 16 == 4 and frames_path(off) == 'strided'
    want = u8_ref(xn, wrap)
    for name, x in (('nchw', xn), ('misaligned', off), ('dense', xd)):
        assert torch.equal(run_frames(x, wrap), want), name


# =================================================================================================================================
# A2. squeeze_rows / squeeze
# =================================================================================================================================
def squeeze_ref(O, x, levels, inverse, cmap, mode):
    """mode 'read': the map acts on the channels of the tensor READ, 'written': of the tensor WRITTEN (cmap: long tensor)"""
    def rep(t, f):
        for _ in range(levels):
            t = f(t)
        return t
    f = O.squeeze_inv if inverse else O.squeeze_fwd
    if mode == 'none':
        return rep(x, f)
    if mode == 'read':
        return rep(x[:, cmap], f)
    y = rep(x, f)
    out = torch.empty_like(y)
    out[:, cmap] = y
    return out


def squeeze_kernel_of(x, out, b, c, h, w, levels, inverse, cmap, map_on_out):
    """the dispatch of ops.squeeze restated: 'rows' (squeeze_rows_kernel) or 'strided' (squeeze_kernel)"""
    fine_side = cmap is None or levels == 0 or (map_on_out == bool(inverse))
    rows = (fine_side and dense_pm(x) and dense_pm(out) and (b * c * h * w) % 4 == 0 and (c << (2 * levels)) % 4 == 0
            and x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0)
    return 'rows' if rows else 'strided'


def squeeze_case(O, dev, b, c, h, w, levels, fine_lay, coarse_lay, mode, seed, counts, big=False):
    """forward and inverse in `mode` against the oracle, then the round trip through the opposite mode; returns nothing, asserts"""
    from sin_inn_amd import ops
    f = 1 << levels
    cc = c * f * f
    fshape, cshape = (b, c, h, w), (b, cc, h // f, w // f)
    g = gen(seed)
    fperm = torch.randperm(c, device=dev, generator=g)
    cperm = torch.randperm(cc, device=dev, generator=g)
    x = Buf(fshape, fine_lay, dev).put(torch.randn(fshape, device=dev, generator=g))
    tag = f'C {c} L {levels} {fine_lay}->{coarse_lay} map {mode}'
    # ---- forward: the map is on the fine side when READ, on the coarse side when WRITTEN
    fmap = {'none': None, 'read': fperm, 'written': cperm}[mode]
    fm32 = fmap.to(torch.int32) if fmap is not None else None
    y = Buf(cshape, coarse_lay, dev)
    counts[squeeze_kernel_of(x.t, y.t, b, c, h, w, levels, False, fm32, mode == 'written')] += 1
    ops.squeeze(x.t, y.t, b, c, h, w, levels, False, fm32, mode == 'written')
    want = squeeze_ref(O, x.t, levels, False, fmap, mode)
    assert torch.equal(y.t, want), tag + ' forward'
    assert y.clean() and x.clean(), tag + ' forward wrote outside its rows'
    y2 = Buf(cshape, coarse_lay, dev)
    ops.squeeze(x.t, y2.t, b, c, h, w, levels, False, fm32, mode == 'written')
    assert same_bits(y2.flat, y.flat), tag + ' forward twice'
    # ---- round trip: the inverse with the SAME map on the same side, i.e. in the opposite mode
    back_mode = {'none': 'none', 'read': 'written', 'written': 'read'}[mode]
    xb = Buf(fshape, fine_lay, dev)
    counts[squeeze_kernel_of(y.t, xb.t, b, c, h, w, levels, True, fm32, back_mode == 'written')] += 1
    ops.squeeze(y.t, xb.t, b, c, h, w, levels, True, fm32, back_mode == 'written')
    assert torch.equal(xb.t, x.t), tag + ' round trip'
    assert xb.clean(), tag + ' inverse wrote outside its rows'
    if big:
        return
    # ---- inverse in `mode` of a fresh coarse tensor: the map is on the coarse side when READ, on the fine side when WRITTEN
    imap = {'none': None, 'read': cperm, 'written': fperm}[mode]
    im32 = imap.to(torch.int32) if imap is not None else None
    z = Buf(cshape, coarse_lay, dev).put(torch.randn(cshape, device=dev, generator=g))
    xi = Buf(fshape, fine_lay, dev)
    counts[squeeze_kernel_of(z.t, xi.t, b, c, h, w, levels, True, im32, mode == 'written')] += 1
    ops.squeeze(z.t, xi.t, b, c, h, w, levels, True, im32, mode == 'written')
    assert torch.equal(xi.t, squeeze_ref(O, z.t, levels, True, imap, mode)), tag + ' inverse'
    assert xi.clean(), tag + ' inverse wrote outside its rows'


@pytest.mark.parametrize('c', [3, 12, 48])
def test_squeeze_levels_0_to_4_every_map_side(dev, O, c):
    """2 x C x 32 x 48, levels 0 .. 4, forward / inverse / round trip, no map, map on the side read, map on the side written,
    dense pixel-major on both sides (squeeze_rows where its conditions hold: C = 3 is its non-vector gather, a map too; C = 12 and
    48 without a map its 16-byte gather) and NCHW or padded rows on one side (squeeze_kernel, x_fastest 1 and 0)"""
    counts = {'rows': 0, 'strided': 0}
    for levels in range(5):
        for fine_lay, coarse_lay in (('pm', 'pm'), ('nchw', 'pm'), ('pmpad', 'pm'), ('pm', 'nchw')):
            for mode in ('none', 'read', 'written'):
                squeeze_case(O, dev, 2, c, 32, 48, levels, fine_lay, coarse_lay, mode, 100 * levels + c, counts)
    print(f'C {c}: launches {counts}')
    assert counts['rows'] >= (20 if c % 4 == 0 else 16) and counts['strided'] >= 100


# name: (shape, levels, map mode, cap property)
SQUEEZE_ROWS_BIG = {'c3_l1_map': ((24, 3, 512, 512), 1, 'read'), 'c3_l2_map': ((24, 3, 512, 512), 2, 'read'),
                    'c12_l2_vec': ((6, 12, 512, 512), 2, 'none')}


@pytest.mark.parametrize('case', sorted(SQUEEZE_ROWS_BIG))
def test_squeeze_rows_past_its_cap(dev, O, case):
    """16384 blocks x 256 threads x 4 floats = 16 777 216 floats a sweep.  The map rides on the fine side: read in the forward, written
    (through its inverse permutation) in the round trip."""
    (b, c, h, w), levels, mode = SQUEEZE_ROWS_BIG[case]
    p = plan(f'squeeze_rows {case}', b * c * h * w // 4, 16384, per_thread=4)
    assert past_cap(p, 16384), p
    counts = {'rows': 0, 'strided': 0}
    squeeze_case(O, dev, b, c, h, w, levels, 'pm', 'pm', mode, 7, counts, big=True)
    assert counts == {'rows': 2, 'strided': 0}, counts


# name: (shape, levels, fine layout, coarse layout, map mode)
SQUEEZE_STRIDED_BIG = {
    'configs3_fine_nchw_read': ((16, 3, 512, 512), 2, 'nchw', 'pm', 'read'),            # x_fastest 1
    'configs3_fine_nchw_written': ((16, 3, 512, 512), 2, 'nchw', 'pm', 'written'),
    'configs3_fine_padded_written': ((16, 3, 512, 512), 2, 'pmpad', 'pm', 'written'),   # x_fastest 0
    'ragged_fine_padded_read': ((5, 3, 516, 548), 2, 'pmpad', 'pm', 'read'),
    'ragged_coarse_nchw_written': ((5, 3, 516, 548), 1, 'pm', 'nchw', 'written'),
}


@pytest.mark.parametrize('case', sorted(SQUEEZE_STRIDED_BIG))
def test_squeeze_strided_past_its_cap(dev, O, case):
    """squeeze_kernel: 16384 blocks x 256 = 4 194 304 elements a sweep.  configs[3]'s own input, 16 x 3 x 512 x 512, is exactly three
    sweeps; the 5 x 3 x 516 x 548 cases end in a partial trip."""
    (b, c, h, w), levels, fine_lay, coarse_lay, mode = SQUEEZE_STRIDED_BIG[case]
    p = plan(f'squeeze {case}', b * c * h * w, 16384)
    assert p['blocks'] == 16384 and p['trips'] >= 2, p
    if case.startswith('ragged'):
        assert past_cap(p, 16384), p
    counts = {'rows': 0, 'strided': 0}
    squeeze_case(O, dev, b, c, h, w, levels, fine_lay, coarse_lay, mode, 8, counts, big=True)
    assert counts == {'rows': 0, 'strided': 2}, counts
    print(f'  x_fastest = {1 if fine_lay == "nchw" else 0}')


# =================================================================================================================================
# A3. permute_channels
# =================================================================================================================================
def test_permute_channels_past_its_cap_strided_rows(dev):
    from sin_inn_amd import ops
    M, C, si, so = 16 * 64 * 64 + 5, 96, 104, 100
    p = plan('permute_channels', M * C, 16384)
    assert past_cap(p, 16384), p
    g = gen(11)
    xin = torch.randn(M, si, device=dev, generator=g)
    perm = torch.randperm(C, device=dev, generator=g)
    assert not torch.equal(perm, torch.arange(C, device=dev))
    outs = []
    for _ in range(2):
        buf = torch.full((M * so + GUARD,), float('nan'), device=dev)
        out = buf[:M * so].view(M, so)
        ops.permute_channels(xin[:, :C], out[:, :C], perm.to(torch.int32))
        assert torch.equal(out[:, :C], xin[:, perm])
        assert untouched(out[:, C:]) and untouched(buf[M * so:]), 'gap columns or the guard were written'
        outs.append(buf)
    assert same_bits(outs[0], outs[1])


# =================================================================================================================================
# A4. haar
# =================================================================================================================================
def haar_parts(x):
    return x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]


def haar_fp32(x, inverse):
    """the kernel's own association restated in torch, one rounding per torch op: ((a + b) + c) + d, signs as in haar_kernel"""
    if not inverse:
        a, b, c, d = haar_parts(x)
        return torch.cat((((a + b) + c) + d, ((a - b) + c) - d, ((a + b) - c) - d, ((a - b) - c) + d), 1) * 0.25
    C = x.shape[1] // 4
    ll, b1, b2, b3 = x[:, :C], x[:, C:2 * C], x[:, 2 * C:3 * C], x[:, 3 * C:]
    out = torch.empty((x.shape[0], C, 2 * x.shape[2], 2 * x.shape[3]), device=x.device, dtype=x.dtype)
    out[:, :, 0::2, 0::2] = ((ll + b1) + b2) + b3
    out[:, :, 0::2, 1::2] = ((ll - b1) + b2) - b3
    out[:, :, 1::2, 0::2] = ((ll + b1) - b2) - b3
    out[:, :, 1::2, 1::2] = ((ll - b1) - b2) + b3
    return out


def run_haar(x, out, C, H, W, inverse):
    from sin_inn_amd import _lib, ops
    _lib.check(_lib.lib().sininn_haar(ops.ptr(x), ops.strides4(x), ops.ptr(out), ops.strides4(out), x.shape[0], C, H, W, inverse, ops._stream()))


@pytest.mark.parametrize('inverse', [0, 1], ids=['analysis', 'synthesis'])
@pytest.mark.parametrize('lay_in,lay_out', [('nchw', 'pm'), ('pm', 'nchw'), ('pmpad', 'pmpad'), ('nchw', 'nchw')])
def test_haar_past_its_cap(dev, O, lay_in, lay_out, inverse):
    """16 x 3 x 512 x 512: 3 145 728 coarse elements, 8192 blocks x 256 = 2 097 152 a sweep.  c_fastest follows the COARSE side's
    channel stride.  Bitwise against the fp32 restatement; against the float64 oracle at 3 U (|a| + |b| + |c| + |d|): three adds."""
    B, C, H, W = 16, 3, 512, 512
    fine, coarse = (B, C, H, W), (B, 4 * C, H // 2, W // 2)
    p = plan(f'haar {lay_in}->{lay_out} inverse {inverse}', B * C * (H // 2) * (W // 2), 8192)
    assert past_cap(p, 8192), p
    src_shape, dst_shape = (coarse, fine) if inverse else (fine, coarse)
    x = Buf(src_shape, lay_in, dev).put(torch.randn(src_shape, device=dev, generator=gen(21 + inverse)))
    outs = []
    for _ in range(2):
        out = Buf(dst_shape, lay_out, dev)
        run_haar(x.t, out.t, C, H, W, inverse)
        assert out.clean() and x.clean(), 'haar wrote outside its rows'
        outs.append(out)
    coarse_t = x.t if inverse else outs[0].t
    print(f'  c_fastest = {1 if coarse_t.stride(1) == 1 else 0}')
    assert same_bits(outs[0].flat, outs[1].flat)
    got = outs[0].t
    assert torch.equal(got, haar_fp32(x.t.contiguous(), inverse))
    x64 = x.t.to(F64)
    if inverse:
        want = O.haar_inv(x64)
        C4 = C
        mag = x64[:, :C4].abs() + x64[:, C4:2 * C4].abs() + x64[:, 2 * C4:3 * C4].abs() + x64[:, 3 * C4:].abs()
        bud = torch.empty_like(want)
        for dy in (0, 1):
            for dx in (0, 1):
                bud[:, :, dy::2, dx::2] = 3 * U * mag
    else:
        want = O.haar_fwd(x64)
        a, b, c, d = haar_parts(x64.abs())
        bud = (3 * U * 0.25 * (a + b + c + d)).repeat(1, 4, 1, 1)
    assert ratio(f'haar {lay_in}->{lay_out} inverse {inverse} vs float64', got, want, bud) <= 1


# =================================================================================================================================
# A5 / A6. samplers
# =================================================================================================================================
def byte_table(dev, dtype=torch.float32):
    """x / 255.f for the 256 bytes, divided on the CPU (IEEE), bf16: that quotient rounded to nearest even"""
    return torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(dev).to(dtype)


def bytes_to_float(u8, dtype=torch.float32):
    return byte_table(u8.device, dtype).index_select(0, u8.reshape(-1).to(torch.int32)).view(u8.shape)


def windows_ref(hr_clip, lr_clip, idx, win):
    """clip[idx] / 255 and the frames idx - win .. idx + win of the LR clip side by side (O.gather_window), every frame index
    clamped to the clip"""
    T = hr_clip.shape[0]
    hr = bytes_to_float(hr_clip[idx.long().clamp(0, T - 1)]).permute(0, 3, 1, 2)
    frames = [lr_clip[(idx.long() - win + f).clamp(0, T - 1)] for f in range(2 * win + 1)]
    lr = bytes_to_float(torch.cat(frames, -1)).permute(0, 3, 1, 2)
    return hr, lr


def windows_path(hr_clip, lr_clip, hr_out, lr_out, win):
    """the density predicate of sample_windows_dense_try restated"""
    _, H, W, _ = hr_clip.shape
    ok = (dense_pm(hr_out) and dense_pm(lr_out) and (H * W * 3) % 16 == 0 and hr_clip.data_ptr() % 16 == 0
          and hr_out.data_ptr() % 16 == 0 and lr_out.data_ptr() % 16 == 0 and lr_clip.data_ptr() % 4 == 0)
    return 'dense' if ok else 'strided'


def windows_case(dev, O, n, T, HW, hw, win, idx, lay, want_path, seed):
    from sin_inn_amd import ops
    (H, W), (h, w) = HW, hw
    g = gen(seed)
    hr_clip = torch.randint(0, 256, (T + 1, H, W, 3), device=dev, generator=g, dtype=torch.uint8)[:T]     # + a guard frame
    lr_clip = torch.randint(0, 256, (T + 1, h, w, 4), device=dev, generator=g, dtype=torch.uint8)[:T]
    idx = torch.tensor(idx, device=dev, dtype=torch.int32)
    assert idx.numel() == n
    lrc = (2 * win + 1) * 4
    want_hr, want_lr = windows_ref(hr_clip, lr_clip, idx, win)
    outs = []
    for _ in range(2):
        hr, lr = Buf((n, 3, H, W), lay, dev), Buf((n, lrc, h, w), lay, dev)
        assert windows_path(hr_clip, lr_clip, hr.t, lr.t, win) == want_path
        ops.sample_windows(hr_clip, lr_clip, idx, win, hr.t, lr.t)
        assert torch.equal(hr.t, want_hr) and torch.equal(lr.t, want_lr)
        assert hr.clean() and lr.clean(), 'sample_windows wrote outside its rows'
        outs.append((hr, lr))
    assert same_bits(outs[0][0].flat, outs[1][0].flat) and same_bits(outs[0][1].flat, outs[1][1].flat)
    # the oracle's own gather (python indexing: no clamp) on the samples whose window lies inside the clip
    inside = [k for k, i in enumerate(idx.tolist()) if win <= i <= T - 1 - win][:2]
    assert inside
    lr_cpu, hr_cpu = lr_clip.cpu(), hr_clip.cpu()
    for k in inside:
        h0, l0 = O.gather_window(lr_cpu, hr_cpu, int(idx[k]), win)
        assert torch.equal(want_hr[k].cpu(), h0) and torch.equal(want_lr[k].cpu(), l0)


def test_sample_windows_dense_past_its_cap(dev, O):
    n, T, win = 16, 40, 10
    hr_items, lr_items = n * 512 * 512 * 3 // 16, n * 128 * 128 * (2 * win + 1)
    p = plan('sample_windows dense', hr_items + lr_items, 16384)
    assert past_cap(p, 16384), p
    idx = [0, 3, T - 1, T - 4, -2, T + 1, T, 17, 20, 11, 29, 5, 33, 12, 25, 8]      # clamps at both ends; two outside the clip
    windows_case(dev, O, n, T, (512, 512), (128, 128), win, idx, 'pm', 'dense', 31)


def test_sample_windows_dense_wave_straddles_hr_and_lr(dev, O):
    n, T, win, H, W = 3, 9, 2, 24, 40
    assert (H * W * 3) % 16 == 0
    hr_items = n * H * W * 3 // 16
    plan('sample_windows dense, small', hr_items + n * 6 * 10 * (2 * win + 1), 16384)
    print(f'  hr_items {hr_items}: lanes {hr_items % 64} .. 63 of wave {hr_items // 64} take the LR branch')
    assert hr_items % 64 != 0
    windows_case(dev, O, n, T, (H, W), (6, 10), win, [0, T - 1, 4], 'pm', 'dense', 32)


@pytest.mark.parametrize('case', ['nchw', 'odd_frame_padded_rows'])
def test_sample_windows_strided_past_its_cap(dev, O, case):
    n, T, win = 3, 9, 2
    HW, hw, lay = (((512, 512), (128, 128), 'nchw') if case == 'nchw' else ((510, 514), (127, 129), 'pmpad'))
    total = n * HW[0] * HW[1] * 3 + n * hw[0] * hw[1] * (2 * win + 1) * 4
    p = plan(f'sample_windows strided {case}', total, 8192)
    assert past_cap(p, 8192), p
    if case != 'nchw':
        assert (HW[0] * HW[1] * 3) % 16 != 0
    windows_case(dev, O, n, T, HW, hw, win, [1, T - 1, 4], lay, 'strided', 33)


def test_sample_windows_odd_frame_dense_layout_takes_strided_kernel(dev, O):
    """dense pixel-major outputs, but H * W * 3 % 16 != 0: the frame is no whole number of 16-byte items"""
    assert (510 * 514 * 3) % 16 != 0
    windows_case(dev, O, 3, 9, (510, 514), (127, 129), 2, [0, 8, 4], 'pm', 'strided', 34)


@pytest.mark.parametrize('dtype', [torch.float32, BF], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('gap', [1, 3])
def test_sample_pairs_past_its_cap(dev, gap, dtype):
    from sin_inn_amd import _lib, ops
    from sin_inn_amd.functional import sample_pairs
    n, T, H, W = 9, 12, 1024, 1024
    p = plan('sample_pairs', n * 2 * (H * W // 4), 16384, per_thread=4)
    assert past_cap(p, 16384), p
    clip = torch.randint(0, 256, (T + 1, H, W, 3), device=dev, generator=gen(41), dtype=torch.uint8)[:T]
    idx = torch.tensor([0, 5, T - 1, T - 2, -1, 3, 7, T - 1, 10], device=dev, dtype=torch.int32)
    assert int((idx + gap >= T).sum()) >= 2 and int((idx < 0).sum()) == 1, 'second frames that clamp, one negative index'
    t0 = idx.long().clamp(0, T - 1)
    t1 = (idx.long() + gap).clamp(0, T - 1)
    want0 = bytes_to_float(clip[t0], dtype).permute(0, 3, 1, 2)
    want1 = bytes_to_float(clip[t1], dtype).permute(0, 3, 1, 2)
    numel = n * 3 * H * W
    runs = []
    for _ in range(2):
        bufs = [torch.full((numel + GUARD,), float('nan'), device=dev, dtype=dtype) for _ in range(2)]
        _lib.check(_lib.lib().sininn_sample_pairs(clip.data_ptr(), idx.data_ptr(), n, T, H, W, gap, bufs[0].data_ptr(), bufs[1].data_ptr(),
                                                  int(dtype == BF), ops._stream()))
        for buf, want in zip(bufs, (want0, want1)):
            assert torch.equal(buf[:numel].view(n, 3, H, W), want)
            assert untouched(buf[numel:]), 'sample_pairs wrote past its output'
        runs.append(bufs)
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
    a, b = sample_pairs(clip, idx, gap, dtype)                     # the front end
    assert torch.equal(a, want0) and torch.equal(b, want1)


# =================================================================================================================================
# D. Bayer synthesis (numpy / scipy float64 oracle on the CPU)
# =================================================================================================================================
def run_bayer(entry, hr, out_shape, scale, reduction):
    from sin_inn_amd import _lib, ops
    T, H, W, _ = hr.shape
    n = int(np.prod(out_shape))
    outs = []
    for sentinel in (0xA5, 0x5A):
        buf = torch.full((n + GUARD,), sentinel, device=hr.device, dtype=torch.uint8)
        _lib.check(getattr(_lib.lib(), entry)(hr.data_ptr(), buf.data_ptr(), T, H, W, scale, 1 if reduction == 'sum' else 0, ops._stream()))
        assert bool((buf[n:] == sentinel).all()), entry + ' wrote past its output'
        outs.append(buf[:n].view(out_shape))
    assert torch.equal(outs[0], outs[1]), 'an output byte kept its sentinel, or two calls differ'
    return outs[0].cpu().numpy()


def bayer_clip(T, H, W, seed, divide=1):
    hr = torch.randint(0, 256, (T, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    hr[:, :2, :, :] = 255                                      # saturated and black stripes at the frame border
    hr[:, :, -2:, :] = 0
    return hr // divide


def test_bayer_bin_past_its_cap(dev, O):
    from sin_inn_amd.functional import bayer_bin
    T, H, W = 9, 1024, 1024
    p = plan('bayer_bin', T * (H // 2) * (W // 2) * 4, 8192)
    assert past_cap(p, 8192), p
    hr = bayer_clip(T, H, W, 51)
    want = O.bayer_bin(hr.numpy(), 1, 'mean')
    got = run_bayer('sininn_bayer_bin', hr.to(dev), (T, H // 2, W // 2, 4), 1, 'mean')
    assert np.array_equal(got, want)
    assert np.array_equal(bayer_bin(hr.to(dev), 1, 'mean').cpu().numpy(), want)


def borders_equal(got, want):
    return all(np.array_equal(got[sl], want[sl]) for sl in ((slice(None), 0), (slice(None), -1), (slice(None), slice(None), 0),
                                                           (slice(None), slice(None), -1)))


def test_bayer_demosaic_past_its_cap(dev, O):
    from sin_inn_amd.functional import bayer_demosaic
    T, H, W = 3, 1024, 1024
    p = plan('bayer_demosaic', T * H * W, 8192)
    assert past_cap(p, 8192), p
    hr = bayer_clip(T, H, W, 52)
    want = O.bayer_demosaic(hr.numpy(), 1, 'mean')
    got = run_bayer('sininn_bayer_demosaic', hr.to(dev), (T, H, W, 3), 1, 'mean')
    assert borders_equal(got, want), "the frame border (scipy's reflect)"
    assert np.array_equal(got, want)
    assert np.array_equal(bayer_demosaic(hr.to(dev), 1, 'mean').cpu().numpy(), want)


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
def test_bayer_scale_4_both_reductions(dev, O, reduction):
    T, H, W, scale = 2, 64, 96, 4
    hr = bayer_clip(T, H, W, 53, divide=8 if reduction == 'sum' else 1)
    hn = hr.numpy()
    want = O.bayer_bin(hn, scale, reduction)
    if reduction == 'sum':
        assert (want == 255).any() and (want < 255).any(), 'some sums are clipped, most are not'
    assert np.array_equal(run_bayer('sininn_bayer_bin', hr.to(dev), (T, H // 8, W // 8, 4), scale, reduction), want)
    wd = O.bayer_demosaic(hn, scale, reduction)
    gd = run_bayer('sininn_bayer_demosaic', hr.to(dev), (T, H // 4, W // 4, 3), scale, reduction)
    assert borders_equal(gd, wd), "the frame border (scipy's reflect)"
    assert np.array_equal(gd, wd)


# =================================================================================================================================
# B. coupling tails against float64
# =================================================================================================================================
def test_device_exp_and_atan_error(dev):
    """the library figures of the docstring, measured again (2^24 draws each): they must stay inside the allowances the budgets
    below use.  This measures torch.exp / torch.atan, not the code under test."""
    g = gen(60)
    for name, fn, lo, hi, allow in (('expf', torch.exp, -24.0, 24.0, EXPF_U), ('atanf', torch.atan, -64.0, 64.0, ATANF_U)):
        x = torch.rand(1 << 24, device=dev, generator=g) * (hi - lo) + lo
        r = fn(x.to(F64))
        rel = float(((fn(x).to(F64) - r).abs() / r.abs().clamp_min(1e-300)).max()) / U
        print(f'{name}: worst relative error {rel:.4f} U on [{lo}, {hi}], allowance {allow} U')
        assert rel <= allow


def glow_ref(g, u, s, gl, clamp, inverse):
    """float64 of coupling_bwd_kernel on float64 copies of its fp32 inputs, and the budget of its fp32 evaluation, per element.
      x = s / clamp                      1 rounding
      L = (clamp * 0.636f) * atanf(x)    the constant 1, atanf ATANF_U + 1 (its argument's rounding moves atan by at most U |atan|, since
                                         x / (1 + x^2) <= atan x), the product 1                  -> rL = (ATANF_U + 3) U relative
      e = expf(L)                        EXPF_U U relative, plus |L| rL through d e / d L = e      -> re
      dL = 0.636f / (1 + x * x)          x 1, x * x 2 + 1, the sum 1 (x^2 / (1 + x^2) <= 1), the quotient 1  -> 6 U relative
    forward:  dv = g e [re + 1 U]; dt = g [exact]; ds = (g u e + gl) dL: g u e [re + 2 U], the sum 1 U of |g u e| + |gl|, times dL [7 U]
    inverse:  dv = g / e [re + 1 U]; dt = -dv; ds = -(g y + gl) dL: g y [1 U], the sum 1 U, times dL [7 U]"""
    k, cl = float(np.float32(0.636)), float(np.float32(clamp))
    x = s / cl
    L = cl * k * torch.atan(x)
    dL = k / (1 + x * x)
    e = torch.exp(L)
    rL = (ATANF_U + 3) * U
    re = EXPF_U * U + rL * L.abs()
    if not inverse:
        dv, dt = g * e, g
        t1 = g * u * e
        ds = (t1 + gl) * dL
        Edv, Edt = dv.abs() * (re + U), torch.zeros_like(g)
        Eds = (t1.abs() * (re + 2 * U) + U * (t1.abs() + gl.abs())) * dL + 7 * U * ds.abs()
    else:
        dv = g / e
        dt = -dv
        t1 = g * u
        ds = -(t1 + gl) * dL
        Edv = dv.abs() * (re + U)
        Edt = Edv
        Eds = (U * t1.abs() + U * (t1.abs() + gl.abs())) * dL + 7 * U * ds.abs()
    return (ds, Eds * SECOND), (dt, Edt * SECOND), (dv, Edv * SECOND)


# name: (B, HW, Co)
COUPLING_CASES = {'configs1_co24': (16, 256 * 256, 24), 'ragged_co24': (3, 61 * 67, 24), 'ragged_co96': (5, 149 * 151, 96)}
COUPLING_WORST = {}


@pytest.mark.parametrize('inverse', [0, 1], ids=['forward', 'inverse'])
@pytest.mark.parametrize('case', sorted(COUPLING_CASES))
def test_coupling_bwd_against_float64(dev, case, inverse):
    """8192 blocks x 256 = 2 097 152 quads a sweep: configs[1]'s level-0 half (6 291 456 quads, exactly three sweeps), one block
    row short of a block (ragged_co24), and Co = 96 past the cap with a partial last trip (ragged_co96); with and without the
    channel maps and the log-det gradient; dy / vy rows wider than Co, dv a slot inside wider rows."""
    from sin_inn_amd import ops
    B, HW, Co = COUPLING_CASES[case]
    M = B * HW
    p = plan(f'coupling_bwd {case}', M * (Co // 4), 8192, per_thread=4)
    if case == 'configs1_co24':
        assert p['blocks'] == 8192 and p['trips'] == 3, p
    elif case == 'ragged_co96':
        assert past_cap(p, 8192), p
    else:
        assert p['trips'] == 1 and p['remainder'] != 0, p
    clamp = 2.0
    g0 = gen(61 + inverse)
    wide = 2 * Co + 4                                         # the map's values reach 2 Co - 1
    dyb = torch.randn(M, wide, device=dev, generator=g0)
    vyb = torch.randn(M, wide, device=dev, generator=g0)
    s = 3.0 * torch.randn(M, Co, device=dev, generator=g0)
    gld = torch.randn(B, device=dev, generator=g0)
    cmap = ops.coupling_colmap(Co, dev)[:Co].contiguous()
    assert int(cmap.min()) >= 0 and int(cmap.max()) < wide and not torch.equal(cmap.long(), torch.arange(Co, device=dev))
    # both sides of the soft clamp, both signs, well into its flat part
    share = float((s.abs() > clamp).double().mean())
    print(f'  |s| > clamp for {share:.3g} of the elements; max |s| / clamp {float(s.abs().max()) / clamp:.3g}')
    assert 0.2 < share < 0.8 and bool((s > 3 * clamp).any()) and bool((s < -3 * clamp).any())
    s64 = s.to(F64)
    active = (s.abs() > clamp)
    dv_stride, dv_off = Co + 8, 4
    for use_map in (False, True):
        cols = cmap.long() if use_map else torch.arange(Co, device=dev)
        g64, u64 = dyb[:, cols].to(F64), vyb[:, cols].to(F64)
        mp = ops.ptr(cmap, dtype=torch.int32) if use_map else None
        for use_gld in (False, True):
            gl = gld.to(F64).repeat_interleave(HW)[:, None] if use_gld else torch.zeros(1, 1, device=dev, dtype=F64)
            (ds, Eds), (dt, Edt), (dv, Edv) = glow_ref(g64, u64, s64, gl.expand(M, Co), clamp, inverse)
            runs = []
            for _ in range(2):
                drb = torch.full((M * 2 * Co + GUARD,), float('nan'), device=dev)
                dvb = torch.full((M * dv_stride + GUARD,), float('nan'), device=dev)
                ops.coupling_bwd(dyb, 0, wide, mp, vyb, 0, wide, mp, s, gld if use_gld else None, B, HW, Co, clamp, inverse,
                                 drb, dvb, dv_off, dv_stride)
                runs.append((drb, dvb))
            assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
            dr = drb[:M * 2 * Co].view(M, 2 * Co)
            rows = dvb[:M * dv_stride].view(M, dv_stride)
            assert untouched(drb[M * 2 * Co:]) and untouched(dvb[M * dv_stride:]), 'wrote past the last row'
            assert untouched(rows[:, :dv_off]) and untouched(rows[:, dv_off + Co:]), 'dv wrote outside its slot'
            tag = f'coupling_bwd {case} inverse {inverse} map {int(use_map)} gld {int(use_gld)}'
            r = dict(ds=ratio(tag + ' ds', dr[:, :Co], ds, Eds), dt=ratio(tag + ' dt', dr[:, Co:], dt, Edt),
                     dv=ratio(tag + ' dv', rows[:, dv_off:dv_off + Co], dv, Edv),
                     ds_active=ratio(tag + ' ds where |s| > clamp', dr[:, :Co], ds, Eds, exempt=~active))
            for k, v in r.items():
                COUPLING_WORST[k] = max(COUPLING_WORST.get(k, 0.0), v)
                assert v <= 1, (tag, k, v)
            if not inverse:
                assert torch.equal(dr[:, Co:], dyb[:, cols]), 'dt = dy exactly'
    print(f'  worst so far: {COUPLING_WORST}')


def irn_common(h, clamp):
    """float64 sigma, s = clamp (2 sigma - 1), e = exp(s) and the bounds of their fp32 evaluation, per element.
      E1 = expf(-h)          EXPF_U U relative
      d = 1 + E1             1 rounding; E1's error enters with weight E1 / (1 + E1) = 1 - sigma
      q = 1 / d (or 2 / d)   1 rounding                                         -> rsg = EXPF_U U (1 - sigma) + 2 U relative
      2 q - 1                2 q is exact; the difference rounds once: absolute 2 sigma rsg + U |2 sigma - 1|
      s = clamp * (..)       1 rounding                                         -> ds (absolute)
      e = expf(s)            EXPF_U U relative plus ds through d e / d s = e    -> re"""
    cl = float(np.float32(clamp))
    sg = torch.sigmoid(h)
    om = torch.sigmoid(-h)                                    # 1 - sigma without the cancellation
    s = cl * (sg - om)
    rsg = EXPF_U * U * om + 2 * U
    ds = cl * (2 * sg * rsg + U * (sg - om).abs()) + U * s.abs()
    e = torch.exp(s)
    re = EXPF_U * U + ds
    return cl, sg, om, rsg, e, re


IRN_M, IRN_CO, IRN_CLAMP = 16 * 256 * 256 + 3, 12, 1.0


def irn_inputs(dev, seed):
    g0 = gen(seed)
    h = 3.0 * torch.randn(IRN_M, IRN_CO, device=dev, generator=g0)
    # the saturated ends of the sigmoid (fp32: 1 + expf(-h) == 1 from h ~ 17 on) and its linear middle
    h[::4097, 0], h[1::4097, 1], h[2::4097, 2] = 20.0, -20.0, 0.0
    assert bool((h > 8).any()) and bool((h < -8).any()) and bool((h.abs() < 0.25).any())
    assert bool((1 + torch.exp(-h) == 1).any()), 'a sigmoid that is exactly 1 in fp32'
    return g0, h


@pytest.mark.parametrize('inverse', [0, 1], ids=['forward', 'inverse'])
def test_irn_tail_against_float64(dev, inverse):
    """out = v exp(s) + g [v e: re + 1 U; the sum 1 U of |out|, fused or not] or (v - g) / exp(s) [the difference 1 U, e re, the
    quotient 1 U]; M = 16 * 256 * 256 + 3 pixels of 12 channels: 3 145 737 quads against 2 097 152 a sweep; v and out in wider rows"""
    from sin_inn_amd import _lib, ops
    M, Co = IRN_M, IRN_CO
    p = plan(f'irn_tail inverse {inverse}', M * (Co // 4), 8192, per_thread=4)
    assert past_cap(p, 8192), p
    g0, h = irn_inputs(dev, 71 + inverse)
    vs, os_ = 24, 20
    vb = torch.randn(M, vs, device=dev, generator=g0)
    gg = torch.randn(M, Co, device=dev, generator=g0)
    runs = []
    for _ in range(2):
        ob = torch.full((M * os_ + GUARD,), float('nan'), device=dev)
        _lib.check(_lib.lib().sininn_irn_tail(ops.ptr(vb, 4), vs, ops.ptr(h), ops.ptr(gg), M, Co, IRN_CLAMP, inverse, ops.ptr(ob, 4), os_,
                                              ops._stream()))
        runs.append(ob)
    assert same_bits(runs[0], runs[1])
    rows = ob[:M * os_].view(M, os_)
    assert untouched(ob[M * os_:]) and untouched(rows[:, :4]) and untouched(rows[:, 4 + Co:]), 'irn_tail wrote outside its slot'
    v, g = vb[:, 4:4 + Co].to(F64), gg.to(F64)
    cl, sg, om, rsg, e, re = irn_common(h.to(F64), IRN_CLAMP)
    if not inverse:
        want = v * e + g
        bud = (v * e).abs() * (re + U) + U * want.abs()
    else:
        want = (v - g) / e
        bud = want.abs() * (re + 2 * U)
    assert ratio(f'irn_tail inverse {inverse}', rows[:, 4:4 + Co], want, bud * SECOND) <= 1


@pytest.mark.parametrize('inverse', [0, 1], ids=['forward', 'inverse'])
def test_irn_coupling_bwd_against_float64(dev, inverse):
    """dv = g e or g / e [re + 1 U]; dG = g [exact] or -g / e; dh = gs * ds_dh with gs = g u e [re + 2 U] or -g y [1 U] and
    ds_dh = clamp 2 sigma (1 - sigma): 1 - sigma rounds once and carries sigma's error, absolute sigma rsg + U (1 - sigma) -- where the
    sigmoid saturates that is all of 1 - sigma, and the budget says so; the two products 2 U.  12 582 948 elements, six sweeps of
    8192 x 256; odd row strides (the kernel is scalar)."""
    from sin_inn_amd import _lib, ops
    M, Co = IRN_M, IRN_CO
    p = plan(f'irn_coupling_bwd inverse {inverse}', M * Co, 8192)
    assert past_cap(p, 8192), p
    g0, h = irn_inputs(dev, 81 + inverse)
    dys, vys, dvs = 13, 17, 15
    dyb = torch.randn(M, dys, device=dev, generator=g0)
    vyb = torch.randn(M, vys, device=dev, generator=g0)
    runs = []
    for _ in range(2):
        dG = torch.full((M * Co + GUARD,), float('nan'), device=dev)
        dh = torch.full((M * Co + GUARD,), float('nan'), device=dev)
        dvb = torch.full((M * dvs + GUARD,), float('nan'), device=dev)
        _lib.check(_lib.lib().sininn_irn_coupling_bwd(ops.ptr(dyb, 1), dys, ops.ptr(vyb, 2), vys, ops.ptr(h), M, Co, IRN_CLAMP, inverse,
                                                      ops.ptr(dG), ops.ptr(dh), ops.ptr(dvb, 3), dvs, ops._stream()))
        runs.append((dG, dh, dvb))
    for a, b in zip(*runs):
        assert same_bits(a, b)
    rows = dvb[:M * dvs].view(M, dvs)
    assert untouched(dG[M * Co:]) and untouched(dh[M * Co:]) and untouched(dvb[M * dvs:]), 'wrote past the last row'
    # the slot is columns 3 .. 3 + Co of rows of 15: the gap is columns 0 .. 2 of every row (the last row's slot ends the buffer)
    assert untouched(rows[:, :3]), 'dv wrote outside its slot'
    g, u = dyb[:, 1:1 + Co].to(F64), vyb[:, 2:2 + Co].to(F64)
    cl, sg, om, rsg, e, re = irn_common(h.to(F64), IRN_CLAMP)
    dsdh = cl * 2 * sg * om
    Edsdh = cl * 2 * (sg * (sg * rsg + U * om) + om * sg * rsg) + 3 * U * dsdh
    if not inverse:
        dv, wG, gs = g * e, g, g * u * e
        Edv, EG, Egs = dv.abs() * (re + U), torch.zeros_like(g), (g * u * e).abs() * (re + 2 * U)
    else:
        dv = g / e
        wG, gs = -dv, -g * u
        Edv = dv.abs() * (re + U)
        EG, Egs = Edv, U * gs.abs()
    wh = gs * dsdh
    Eh = Egs * dsdh + gs.abs() * Edsdh + U * wh.abs()
    tag = f'irn_coupling_bwd inverse {inverse}'
    assert ratio(tag + ' dv', rows[:, 3:3 + Co], dv, Edv * SECOND) <= 1
    assert ratio(tag + ' dG', dG[:M * Co].view(M, Co), wG, EG * SECOND) <= 1
    got_h = dh[:M * Co].view(M, Co)
    assert ratio(tag + ' dh', got_h, wh, Eh * SECOND) <= 1
    sat = (h.abs() > 8)
    assert ratio(tag + ' dh where the sigmoid saturates', got_h, wh, Eh * SECOND, exempt=~sat) <= 1


# =================================================================================================================================
# C. weight packs against the documented layouts
# =================================================================================================================================
WINO_G = [[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]]


def wino_u(g):
    """U = G g G^T of [..., 3, 3] float64 filters -> [..., 16], and sum |g|"""
    G = torch.tensor(WINO_G, device=g.device, dtype=F64)
    return (G @ g @ G.t()).reshape(*g.shape[:-2], 16), g.abs().sum((-1, -2))


def pack_colmap(n, dev, seed):
    """a packed-column map longer than N: a permutation of the outputs with entries outside [0, N) among them"""
    g = gen(seed)
    m = torch.cat((torch.randperm(n, device=dev, generator=g), torch.tensor([-1, n, n + 5, -7] * 4, device=dev)))
    return m[torch.randperm(m.numel(), device=dev, generator=g)].to(torch.int32).contiguous()


@pytest.mark.parametrize('with_map', [False, True], ids=['nomap', 'colmap'])
@pytest.mark.parametrize('n,cin', [(256, 24), (48, 256), (192, 256)])
def test_pack_conv_matches_documented_layouts(dev, n, cin, with_map):
    """ops.pack_conv's outputs against the layouts documented above pack_winograd_kernel / in ops.pack_conv:
      w_fwd   [9][Np][Cin]          = w[colmap[q]][c][tap]                    bitwise; 0 where colmap[q] is outside [0, N)
      b_fwd   [Np]                  = bias[colmap[q]]                         bitwise
      w_dgrad [9][pad16(Cin)][N]    = w[n][c][8 - tap]                        bitwise; 0 for c >= Cin
      u_fwd   [16][Cin/8][Np][8]    = (G g G^T)[pos], g = w[colmap[q]][c]     4 U sum |g|: two stages of two adds; the 0.5 is exact
      u_dgrad [16][N/8][pad32(Cin)][8] = (G g G^T)[pos], g[a][b] = w[n][c][2-a][2-b]
    pads exactly zero.  Also the 1x1 direct packs."""
    from sin_inn_amd import ops
    g0 = gen(91)
    cmap = pack_colmap(n, dev, 92 + n) if with_map else None
    npk = cmap.numel() if with_map else ops.pad16(n)
    src = cmap.long() if with_map else torch.arange(n, device=dev)
    ok = (src >= 0) & (src < n)
    if with_map:
        assert npk > n and int((~ok).sum()) == 16
    for k in (3, 1):
        taps = k * k
        w = torch.randn(n, cin, k, k, device=dev, generator=g0)
        b = torch.randn(n, device=dev, generator=g0)
        wsel = torch.where(ok[:, None, None], w.reshape(n, cin, taps)[src.clamp(0, n - 1)], torch.zeros((), device=dev))    # [Np][Cin][taps]
        for wino in ((False, True) if k == 3 else (False,)):
            cdp = ops.pad32(cin) if wino else ops.pad16(cin)
            sizes = ((16 if wino else taps) * npk * cin, npk, (16 if wino else taps) * cdp * n)
            bufs = [torch.full((sz + GUARD,), float('nan'), device=dev) for sz in sizes]
            out = tuple(bf[:sz] for bf, sz in zip(bufs, sizes))
            ops.pack_conv(w, b, cmap, True, wino, wino, out=out)
            for bf, sz in zip(bufs, sizes):
                assert untouched(bf[sz:]) and bool(torch.isfinite(bf[:sz]).all()), 'a pack wrote past its end or left an element'
            w_fwd, b_fwd, w_dg = out
            assert torch.equal(b_fwd, torch.where(ok, b[src.clamp(0, n - 1)], torch.zeros((), device=dev)))
            tag = f'pack N {n} Cin {cin} k {k} map {int(with_map)}'
            if not wino:
                assert torch.equal(w_fwd.view(taps, npk, cin), wsel.permute(2, 0, 1)), tag + ' w_fwd'
                want = torch.zeros(taps, cdp, n, device=dev)
                want[:, :cin] = w.reshape(n, cin, taps).flip(-1).permute(2, 1, 0)
                assert torch.equal(w_dg.view(taps, cdp, n), want), tag + ' w_dgrad'
                continue
            # Winograd forward pack
            u, mag = wino_u(wsel.to(F64).view(npk, cin, 3, 3))                                 # [Np][Cin][16]
            want = u.view(npk, cin // 8, 8, 16).permute(3, 1, 0, 2)                              # [16][Cin/8][Np][8]
            bud = (4 * U * mag).view(npk, cin // 8, 8).permute(1, 0, 2).expand(16, cin // 8, npk, 8)
            got = w_fwd.view(16, cin // 8, npk, 8)
            assert ratio(tag + ' u_fwd', got, want, bud) <= 1
            assert bool((got[:, :, ~ok] == 0).all()), tag + ' u_fwd pad columns'
            # Winograd data-gradient pack: flipped taps, channel roles swapped, rows c >= Cin zero
            gf = torch.zeros(n, cdp, 3, 3, device=dev, dtype=F64)
            gf[:, :cin] = w.to(F64).flip(-1, -2)
            u, mag = wino_u(gf)                                                                  # [N][Cdp][16]
            want = u.view(n // 8, 8, cdp, 16).permute(3, 0, 2, 1)                                # [16][N/8][Cdp][8]
            bud = (4 * U * mag).view(n // 8, 8, cdp).permute(0, 2, 1).expand(16, n // 8, cdp, 8)
            got = w_dg.view(16, n // 8, cdp, 8)
            assert ratio(tag + ' u_dgrad', got, want, bud) <= 1
            if cdp > cin:
                assert bool((got[:, :, cin:] == 0).all()), tag + ' u_dgrad pad rows'
            # positions 0, 3, 12, 15 of U are single filter taps: exact
            for pos, (a, bb) in ((0, (0, 0)), (3, (0, 2)), (12, (2, 0)), (15, (2, 2))):
                assert torch.equal(w_fwd.view(16, cin // 8, npk, 8)[pos].permute(1, 0, 2).reshape(npk, cin), wsel.view(npk, cin, 3, 3)[:, :, a, bb])
