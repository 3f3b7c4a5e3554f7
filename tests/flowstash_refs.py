"""float64 reference of `flowtrainer.error_stash` and the error budgets its tests hold the kernels to.

    E[b][y][x]         = 0.5 (mean_c |m1 S1 - m1 I1| + mean_c |m2 S2 - m2 I2|)                  float64, from the fp32 inputs
    log_buffer[cell]  += sum of alpha(p, k) E[p] over the points p and corners k with cell(p, k) == cell
    log_counter[cell] += the same sum of alpha(p, k)

The cells and alphas are the fp32 expressions of `StashedSpatialController.cells` restated per axis (the floor and the ceil must decide
as they do in fp32; the kernels clamp an index to the grid, so does this); the accumulation is index_add_ in float64.

Budgets, in units of U = 2^-24, all relative: every term is non-negative, so no absolute term is needed.
  E_ROUNDINGS   the masks of a step are 0 / 1 (an occlusion mask times `splat != 0`), so m S and m I are exact.  Then per direction one
                rounding for each channel's difference, two for the sum of three channels, one for the division by C, and one for the
                sum of the two directions; the factor 0.5 is exact.  Five roundings, (1 + U)^5 - 1 < 6 U.
  STASH_C       what a term of a cell's sum deviates by before any addition: E (5 roundings), the three products a_x E, a_y (.), a_t (.)
                of the kernels (3), the two roundings of the reference's own fp32 alpha = (a_t a_y) a_x (2), the addition to the buffer
                (1), one spare for second-order terms: 12.  The additions themselves: a sum of n non-negative terms in ANY order is
                within (n - 1) U of the exact sum, whence the per-cell budget (n_terms + STASH_C) U reference.  The counter's terms
                carry fewer roundings and the same bound holds.
"""
import torch

U = 2.0 ** -24
E_ROUNDINGS = 6
STASH_C = 12
F64 = torch.float64


def error_map(s1, i1, m1, s2, i2, m2):
    """E (B, H, W) in float64 from the fp32 inputs"""
    def direction(s, i, m):
        s, i, m = s.to(F64), i.to(F64), m.to(F64)
        return (m * s - m * i).abs().mean(1)
    return 0.5 * (direction(s1, i1, m1) + direction(s2, i2, m2))


def axis_cells(v, d, res, centre_scale):
    """one axis of `cells` in fp32: ((lower cell, upper cell) int64, (weight of the lower, of the upper) fp32) of coordinates v (n,)"""
    assert v.dtype == torch.float32
    x = (v - centre_scale[d]) * centre_scale[3 + d]
    u = ((x + 1) / 2) * max(res - 2, 1) + .5
    lo, hi = torch.floor(u), torch.ceil(u + 1e-6)
    return (lo.long().clamp(0, res - 1), hi.long().clamp(0, res - 1)), (hi - u, u - lo)


def corners(times, ys, xs, res, centre_scale):
    """(cells (8, B, H, W) int64, alphas (8, B, H, W) fp32): corner k takes t's upper cell with bit 2, y's with bit 1, x's with bit 0;
    alpha = (a_t a_y) a_x in fp32 and cell = i_t + res (i_y + res i_x), as flat_inds forms them"""
    (it, at), (iy, ay), (ix, ax) = (axis_cells(v, d, res, centre_scale) for d, v in enumerate((times, ys, xs)))
    cells, alphas = [], []
    for k in range(8):
        st, sy, sx = (k >> 2) & 1, (k >> 1) & 1, k & 1
        cells.append(it[st][:, None, None] + res * (iy[sy][None, :, None] + res * ix[sx][None, None, :]))
        alphas.append((at[st][:, None, None] * ay[sy][None, :, None]) * ax[sx][None, None, :])
    return torch.stack(cells), torch.stack(alphas)


def stash(e64, times, ys, xs, res, centre_scale):
    """(log_buffer, log_counter, n_terms), each (res^3,): what one call adds to zeroed logs, in float64, and the number of (point, corner)
    pairs of every cell"""
    cells, alphas = corners(times, ys, xs, res, centre_scale)
    flat = cells.flatten()
    buf = torch.zeros(res ** 3, dtype=F64, device=e64.device).index_add_(0, flat, (alphas.to(F64) * e64[None]).flatten())
    cnt = torch.zeros(res ** 3, dtype=F64, device=e64.device).index_add_(0, flat, alphas.to(F64).flatten())
    return buf, cnt, torch.bincount(flat, minlength=res ** 3)


def check_logs(got_buf, got_cnt, ref_buf, ref_cnt, n_terms, calls=1, mult=1.0, what=''):
    """per cell |got - calls * ref| <= mult (n_terms + STASH_C) U (calls * ref): every call's own sum is within (n_terms + STASH_C - 1) U of
    its reference and the addition to the buffer is one more rounding of the total.  Cells the reference leaves at 0 are exactly 0"""
    for name, got, ref in (('log_buffer', got_buf, ref_buf), ('log_counter', got_cnt, ref_cnt)):
        ref = ref * calls
        budget = mult * (n_terms.to(F64) + STASH_C) * U * ref
        err = (got.to(F64) - ref).abs()
        worst = float((err / budget.clamp_min(1e-300)).max())
        print(f'{what} {name}: worst error / budget {worst:.3f}, cells hit {int((n_terms > 0).sum())} / {n_terms.numel()}')
        assert bool((err <= budget).all()), (what, name, worst)
        assert bool((got[ref == 0] == 0).all()), (what, name, 'a cell the reference leaves at 0 is not 0')
