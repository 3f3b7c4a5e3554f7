"""TEST INFRASTRUCTURE: inputs and the float64 reference of the warp edge tests (tests/test_flowwarp_edges_host.py,
tests/test_gpu_flowwarp_edges.py).  Torch on the CPU only.

The rule under test.  With (ix, iy) the sampling coordinate as `resample2d_coord` / `affine_src` give it in fp32, a pixel has NO
FOOTPRINT when a coordinate is not finite or |ix| >= 1e9 or |iy| >= 1e9.  Its warped value is 0 in every channel, its metric is
mean_c |target|, its gflow is 0 and it adds nothing to gimg.  A huge coordinate below the guard (flows of 5e8, 1e6) keeps its footprint:
its four taps are outside the frame, so it gives the same outputs.

    flow_case(name)      the flow field of one shape: clean pixels with planted pixels among them, and where they are
    coords32 / coords64  the Resample2d coordinate by the kernel's formula in fp32, and in float64 on the same fp32 flow
    no_footprint         the rule, on the fp32 coordinates
    sanitised            float64 coordinates in which every planted pixel samples at OUTSIDE (four taps outside the frame: value 0,
                         no slope, nothing scattered), so a plain 4-tap gather states the rule
    warp64, metric64     the float64 reference of the forward
    affine_thetas        the three thetas of the affine case; affine_coords32 the kernel's formula in fp32

Clean pixels: the float64 coordinate is chosen first, fractional parts in [FRAC_LO, FRAC_HI] within [0.2, 0.8] on both axes, and
`resample2d_coord` is inverted for the flow, which is then rounded to fp32.  The coordinate error of fp32 (about 6 U (|ix| + W)) is far
below 0.2, so fp32 and float64 agree on the cell of every clean pixel and no comparison exempts any.

The share hazard.  The guarded kernels give a lane without a footprint the taps of coordinate (0, 0), north-west tap (y0, x0) = (0, 0).
`flow_warp_l1_kernel` takes its east taps from the next lane when that lane's north-west tap is (y0, x0 + 1).  So the pair that would
match this sentinel is a clean pixel with footprint (0, -1) whose right-hand neighbour has no footprint: SHARE_CLEAN = (1, 0), which
samples at SHARE_COORD = (ix, iy) = (-0.6, 0.5) (a flow of about (-0.1, -0.05)), and SHARE_BAD = (1, 1).
"""
import math

import torch

F64 = torch.float64
U = 2.0 ** -24
GUARD = 1e9
NAN, INF = float('nan'), float('inf')
NO_FOOTPRINT_VALUES = (NAN, INF, -INF, 3e9, -2e9, 1e30, -3.4e38)
HUGE_VALUES = (5e8, 1e6)                                     # below the guard: the footprint stays, all four taps outside
VALUES = NO_FOOTPRINT_VALUES + HUGE_VALUES                   # the cycle of the planted pixels
FRAC_LO, FRAC_HI = 0.21, 0.79
OUTSIDE = -10.0
FB_TX, FB_TY, FB_R = 32, 8, 8                                # tile and LDS window margin of flow_warp_l1_bwd_tiled_kernel
SHARE_CLEAN, SHARE_BAD = (1, 0), (1, 1)
SHARE_COORD = (-0.6, 0.5)

# name -> (B, C, H, W).  ragged: 1710 pixels (a last wave with dead lanes), tiles ragged on both axes.  pass2: C = 5 > 4, the second
# channel pass of the tiled window.
SHAPES = {'ragged': (2, 3, 19, 45), 'pass2': (1, 5, 37, 75)}
AFFINE_SHAPE = (3, 3, 19, 45)


def _towards_centre(pos, n, k):
    """pos + k if that stays a cell with both taps inside an axis of length n, else pos - k; None if neither does"""
    hi, lo = pos + k, pos - k
    ok_hi, ok_lo = hi <= n - 2, lo >= 0
    if ok_hi and (pos < n / 2 or not ok_lo):
        return hi
    return lo if ok_lo else None


def clean_coordinates(B, H, W, seed):
    """float64 (ix, iy) of every pixel, three kinds mixed inside the waves:
      far    (x + y) % 3 == 0 outside the band: the cell is displaced by 9..40 pixels on one axis, inside the frame where the frame has
             room on either axis (taps outside the tiled backward's LDS window), else it stays a sub-pixel;
      leave  the band of two rows in the middle: the cell straddles the left border, the right border, or lies 50 pixels outside;
      sub    everything else: the cell of the zero-flow coordinate, so the motion is below one pixel."""
    g = torch.Generator().manual_seed(seed)
    frac = FRAC_LO + (FRAC_HI - FRAC_LO) * torch.rand(B, 2, H, W, generator=g, dtype=F64)
    disp = torch.randint(9, 41, (B, H, W), generator=g)
    axis = torch.randint(0, 2, (B, H, W), generator=g)
    cx = torch.zeros(B, H, W, dtype=F64)
    cy = torch.zeros(B, H, W, dtype=F64)
    band = (H // 2, H // 2 + 2)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                x0, y0 = math.floor(x * W / (W - 1) - 0.5), math.floor(y * H / (H - 1) - 0.5)
                if band[0] <= y < band[1]:
                    x0 = (-1, W - 1, W + 50)[x % 3]
                elif (x + y) % 3 == 0:
                    k = int(disp[b, y, x])
                    for a in (('y', 'x') if int(axis[b, y, x]) else ('x', 'y')):          # the other axis if this one has no room
                        moved = _towards_centre(y0, H, k) if a == 'y' else _towards_centre(x0, W, k)
                        if moved is not None:
                            x0, y0 = (x0, moved) if a == 'y' else (moved, y0)
                            break
                cx[b, y, x], cy[b, y, x] = x0, y0
    return cx + frac[:, 0], cy + frac[:, 1]


def invert_coordinates(ix, iy, H, W):
    """the fp32 flow whose Resample2d coordinate is (ix, iy): ix = (x + fx) W / (W - 1) - 1/2"""
    xs = torch.arange(W, dtype=F64)[None, None, :]
    ys = torch.arange(H, dtype=F64)[None, :, None]
    fx = (ix + 0.5) * (W - 1) / W - xs
    fy = (iy + 0.5) * (H - 1) / H - ys
    return torch.stack((fx, fy), 1).to(torch.float32).contiguous()


def planted_sites(B, H, W):
    """[(b, y, x, bad_x, bad_y)]: where a value of the cycle is planted, and in which component"""
    def at(flat):
        return (0, flat // W, flat % W)
    sites = [at(0), (B - 1, H - 1, W - 1)]                               # pixel 0; the pixel the forward's dead lanes clone
    sites += [at(63), at(64), at(255), at(256)]                          # a wave boundary; a block boundary of the 256-thread kernels
    sites += [(0, FB_TY - 1, FB_TX - 1), (0, FB_TY, FB_TX)]              # tile corners of the 32 x 8 tiled backward
    sites += [(0, 12, 10), (0, 12, 11), (0, 12, 12)]                     # a bad pixel with bad neighbours
    sites = [s + (True, True) for s in sites]
    sites += [(0, 14, 20, True, False), (0, 14, 30, False, True)]        # only fx; only fy
    sites += [(0,) + SHARE_BAD + (True, True)]
    assert len({s[:3] for s in sites}) == len(sites)
    return sites


def flow_case(name, seed=5):
    """dict: flow (B,2,H,W) fp32, zeroed (the same with the planted flows set to 0), planted (B,H,W) bool, sites [(b,y,x,vx,vy)]"""
    B, C, H, W = SHAPES[name]
    ix, iy = clean_coordinates(B, H, W, seed)
    y, x = SHARE_CLEAN
    ix[0, y, x], iy[0, y, x] = SHARE_COORD
    flow = invert_coordinates(ix, iy, H, W)
    planted = torch.zeros(B, H, W, dtype=torch.bool)
    sites = []
    for i, (b, y, x, bad_x, bad_y) in enumerate(planted_sites(B, H, W)):
        # the single-component sites and the share neighbour take the no-footprint values, so each of them tests what it is there for
        pool = VALUES if (bad_x and bad_y and (y, x) != SHARE_BAD) else NO_FOOTPRINT_VALUES
        v = pool[i % len(pool)]
        if bad_x:
            flow[b, 0, y, x] = v
        if bad_y:
            flow[b, 1, y, x] = v
        planted[b, y, x] = True
        sites.append((b, y, x, v if bad_x else None, v if bad_y else None))
    zeroed = torch.where(planted[:, None], torch.zeros_like(flow), flow)
    return dict(shape=(B, C, H, W), flow=flow, zeroed=zeroed, planted=planted, sites=sites)


def coords32(flow, H, W):
    """`resample2d_coord` of csrc/bilinear_taps.h, operation by operation in fp32 (the planted values are nowhere near the guard, so a
    contracted multiply-add cannot change the side they fall on)"""
    f = flow.to(torch.float32)
    xs = torch.arange(W, dtype=torch.float32)[None, None, :]
    ys = torch.arange(H, dtype=torch.float32)[None, :, None]
    gxn = (xs + f[:, 0]) / float(W - 1) * 2.0 - 1.0
    gyn = (ys + f[:, 1]) / float(H - 1) * 2.0 - 1.0
    return ((gxn + 1.0) * W - 1.0) * 0.5, ((gyn + 1.0) * H - 1.0) * 0.5


def coords64(flow, H, W):
    f = flow.to(F64)
    xs = torch.arange(W, dtype=F64)[None, None, :]
    ys = torch.arange(H, dtype=F64)[None, :, None]
    return (xs + f[:, 0]) * W / (W - 1) - 0.5, (ys + f[:, 1]) * H / (H - 1) - 0.5


def no_footprint(ix32, iy32):
    """the rule; NaN fails both comparisons"""
    return ~((ix32.abs() < GUARD) & (iy32.abs() < GUARD))


def sanitised(flow, planted, H, W):
    """float64 coordinates of `flow` with every planted pixel moved to OUTSIDE"""
    ix, iy = coords64(torch.where(planted[:, None], torch.zeros_like(flow), flow), H, W)
    out = torch.full_like(ix, OUTSIDE)
    return torch.where(planted, out, ix), torch.where(planted, out, iy)


def taps64(img, ix, iy):
    """the 4-tap gather in float64, zeros outside: [(tap value [B,C,H,W], weight [B,H,W], inside [B,H,W], y index, x index)]"""
    B, C, H, W = img.shape
    x0, y0 = ix.floor(), iy.floor()
    wx1, wy1 = ix - x0, iy - y0
    x0, y0 = x0.long(), y0.long()
    flat = img.to(F64).reshape(B, C, H * W)
    out = []
    for dy, dx, w in ((0, 0, (1 - wy1) * (1 - wx1)), (0, 1, (1 - wy1) * wx1), (1, 0, wy1 * (1 - wx1)), (1, 1, wy1 * wx1)):
        yy, xx = y0 + dy, x0 + dx
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(B, 1, H * W).expand(B, C, H * W)
        out.append((flat.gather(2, idx).reshape(B, C, H, W) * inside[:, None], w, inside, yy, xx))
    return out


def warp64(img, flow):
    """the rule written out: the float64 gather where the fp32 coordinate has a footprint, 0 elsewhere"""
    B, C, H, W = img.shape
    bad = no_footprint(*coords32(flow, H, W))
    ix, iy = coords64(torch.where(bad[:, None], torch.zeros_like(flow), flow), H, W)
    val = sum(t * w[:, None] for t, w, _, _, _ in taps64(img, ix, iy))
    return torch.where(bad[:, None], torch.zeros_like(val), val)


def metric64(target, warped):
    return (target.to(F64) - warped.to(F64)).abs().mean(1, keepdim=True)


def window_census(ix, iy, keep):
    """(taps dropped outside the frame, in-frame taps outside the tiled backward's LDS window) over the pixels of `keep`"""
    B, H, W = ix.shape
    xs = torch.arange(W)[None, None, :]
    ys = torch.arange(H)[None, :, None]
    bx0, by0 = xs // FB_TX * FB_TX, ys // FB_TY * FB_TY
    dropped = far = 0
    for _, _, inside, yy, xx in taps64(torch.zeros(B, 1, H, W, dtype=F64), ix, iy):
        qx, qy = xx - (bx0 - FB_R), yy - (by0 - FB_R)
        in_window = (qx >= 0) & (qx < FB_TX + 2 * FB_R) & (qy >= 0) & (qy < FB_TY + 2 * FB_R)
        dropped += int((~inside & keep).sum())
        far += int((inside & ~in_window & keep).sum())
    return dropped, far


# ---- affine ----

def affine_thetas(H, W):
    """(3, 2, 3) fp32.  Sample 0: a theta as tcr.py builds it, rotated by 35 degrees and shifted by a third of the width, so a visible
    share of its taps leaves the frame.  Sample 1: tcr.py's default draw with NaN in theta[2].  Sample 2: the same with 1e10 in
    theta[5]."""
    from tcr import normalized_inverse, pixel_matrix
    big = normalized_inverse(pixel_matrix(torch.tensor([[0.0, 1.0, 0.0]]), H, W, 35.0, W / 3.0, 1), H, W)
    rand = torch.rand(2, 3, generator=torch.Generator().manual_seed(6))
    th = torch.cat((big, normalized_inverse(pixel_matrix(rand, H, W, 5.0, 5.0, 1), H, W)), 0).to(torch.float32)
    th[1, 0, 2] = NAN
    th[2, 1, 2] = 1e10
    return th.contiguous()


def affine_coords32(theta, H, W):
    """`affine_src` of csrc/elementwise.hip in fp32"""
    th = theta.to(torch.float32).reshape(-1, 6)
    xn = ((2.0 * torch.arange(W, dtype=torch.float32) + 1.0) / W - 1.0)[None, None, :]
    yn = ((2.0 * torch.arange(H, dtype=torch.float32) + 1.0) / H - 1.0)[None, :, None]
    t = [th[:, i, None, None] for i in range(6)]
    xs = t[0] * xn + t[1] * yn + t[2]
    ys = t[3] * xn + t[4] * yn + t[5]
    return ((xs + 1.0) * W - 1.0) * 0.5, ((ys + 1.0) * H - 1.0) * 0.5
