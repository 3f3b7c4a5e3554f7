"""GPU: the edges of two operators of csrc/flowtrain.hip -- splat_mask beyond its grid cap and with NaN / infinity in the mask,
flow2img at the block boundaries of its maximum pass, on a 1 x 1 frame, and with a NaN / infinite frame next to clean ones.

splat_mask is compared with `splat_mask_ref` evaluated by torch on the same device: NaN at the same positions, every other element
bitwise equal.  flow2img is compared with `flow2img_ref` under the fixture condition of tests/flowtrainer_refs.py (at most 1 value in
10^4 differs, by one level; on a 1 x 1 frame that allows none), and frames of one batch with the same frames converted alone, bitwise.

Measured on an MI355X (run with -s): splat_mask, cm = 1 and 3: 15 NaN at torch's positions, every other of the 2 163 600 elements
bitwise equal.  flow2img: 0 values differ from the restatement in every image (1 x 1; 2 x 1024 and 1 x 1025 with the largest radius at
pixel 0, 1023, 1024 and the last; the three 3 x 1100 frames, the NaN frame included).  6 tests in 0.2 s.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowtrainer_refs as R  # noqa: E402
from test_gpu_flowtrainer import dev  # noqa: E402,F401
from sin_inn_amd import flowtrainer  # noqa: E402

SPLAT_GRID = 8192 * 256             # elements one sweep of splat_mask_kernel's capped grid covers


# ---- sininn_splat_mask ----

@pytest.mark.parametrize('cm', [1, 3])
def test_splat_mask_beyond_the_grid_cap_with_nan_and_inf(dev, cm):
    """2 163 600 elements against 8192 x 256: the last 66 448 are a block's second trip.  At six pixels the mask is NaN or +inf in
    every channel and the splat is (0, 2, -0) over its three channels: NaN stays NaN whatever the splat, inf * 0 is NaN and inf * 1
    is inf, as torch's `mask * (splat != 0)` gives them."""
    n, c, h, w = 2, 3, 600, 601
    total = n * c * h * w
    assert total > SPLAT_GRID
    g = torch.Generator().manual_seed(14)
    splat = torch.randn(n, c, h, w, generator=g)
    splat[torch.rand(n, c, h, w, generator=g) < 0.2] = 0.0
    splat[0, 1, 2, 3], splat[1, 2, 599, 0], splat[1, 0, 0, 0] = -0.0, -0.0, 0.0
    mask = (torch.rand(n, cm, h, w, generator=g) > 0.3).float() * (1 + torch.rand(n, cm, h, w, generator=g))
    nan, inf = float('nan'), float('inf')
    special = [(nan, 0, 0, 0), (inf, 0, 300, 17), (nan, 1, 500, 3), (inf, 1, 555, 600), (inf, 1, 599, 599), (nan, 1, h - 1, w - 1)]
    for value, s, y, x in special:
        mask[s, :, y, x] = value
        splat[s, :, y, x] = torch.tensor([0.0, 2.0, -0.0])
    flat = [((s * c + ch) * h + y) * w + x for _, s, y, x in special for ch in range(c)]
    assert max(flat) == total - 1 and sum(i >= SPLAT_GRID for i in flat) >= 4, 'the last element and several of the second trip'
    splat, mask = splat.to(dev), mask.to(dev)
    got = flowtrainer.splat_mask(mask, splat)
    want = R.splat_mask_ref(mask, splat)
    assert got.shape == want.shape and got.dtype == torch.float32
    nan_want = torch.isnan(want)
    # what the inputs are for, on the reference alone: 3 NaN pixels x 3 channels, and 3 inf pixels x the 2 channels with a zero splat
    assert int(nan_want.sum()) == 15 and int(torch.isinf(want).sum()) == 3
    assert torch.equal(torch.isnan(got), nan_want), 'NaN at other positions than torch'
    same = got.view(torch.int32) == want.view(torch.int32)
    assert bool((same | nan_want).all()), f'{int((~(same | nan_want)).sum())} elements differ bitwise'
    assert float(got[0, 1, 2, 3]) == 0.0 and float(got[1, 2, 599, 0]) == 0.0


# ---- sininn_flow2img ----

@pytest.mark.parametrize('shape', [(1, 2, 1, 1), (1, 2, 2, 1024), (1, 2, 1, 1025)], ids=['1x1', '2x1024', '1x1025'])
def test_flow2img_at_block_boundaries(dev, shape):
    """1 x 1: one pixel, its own maximum.  2 x 1024: exactly two blocks of the maximum pass.  1 x 1025: one block and one pixel.
    The largest radius is put at the first and last pixel of the frame and on both sides of the block boundary in turn: a block
    or a pixel the maximum pass leaves out changes maxrad and with it the whole image."""
    _, _, h, w = shape
    hw = h * w
    g = torch.Generator().manual_seed(15)
    base = torch.randn(shape, generator=g)
    for peak in sorted({0, 1023, 1024, hw - 1} & set(range(hw))):
        flow = base.clone()
        flow[0, 0].view(-1)[peak], flow[0, 1].view(-1)[peak] = 6.0, -7.0
        got = flowtrainer.flow2img(flow.to(dev))
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 3, h, w)
        R.assert_image_close(got[0].cpu(), R.flow2img_ref(flow[0]), f'{h} x {w}, largest radius at pixel {peak}')


def test_flow2img_keeps_a_nan_frame_apart(dev):
    """three 3 x 1100 frames (four blocks of the maximum pass each); frame 1 holds a NaN, a +inf and a -inf, frames 0 and 2 are clean
    with maxima about 4 and 0.6.  The NaN makes frame 1's maximum NaN and max(-1, nan) = -1 its maxrad, for that frame alone."""
    g = torch.Generator().manual_seed(16)
    frames = torch.randn(3, 2, 3, 1100, generator=g) * torch.tensor([1.0, 2.0, 0.15]).view(3, 1, 1, 1)
    frames[1, 0, 1, 1050] = float('nan')                         # in the third block
    frames[1, 1, 0, 5] = float('inf')
    frames[1, 0, 2, 1099] = float('-inf')                        # the last pixel
    # on the reference alone: the infinities are clipped and maxrad = -1 flips the direction, so frame 1 still shows its flow
    ref1 = R.flow2img_ref(frames[1])
    nan_pixel = torch.isnan(frames[1]).any(0)
    assert int(nan_pixel.sum()) == 1 and not bool(ref1[:, nan_pixel].any()), 'the NaN pixel is black'
    assert bool((ref1[:, ~nan_pixel] != 0).any(0).float().mean() > 0.5), 'frame 1 is not black outside its NaN pixel'
    cleaned = frames.clone()
    cleaned[1] = 0.0
    frames, cleaned = frames.to(dev), cleaned.to(dev)
    batch, batch_cleaned = flowtrainer.flow2img(frames), flowtrainer.flow2img(cleaned)
    assert tuple(batch.shape) == (3, 3, 3, 1100)
    for i in range(3):
        single = flowtrainer.flow2img(frames[i])
        assert torch.equal(batch[i], single), f'frame {i} in the batch is not frame {i} alone'
        R.assert_image_close(single.cpu(), ref1 if i == 1 else R.flow2img_ref(frames[i].cpu()), f'frame {i} against the restatement')
    for i in (0, 2):
        assert torch.equal(batch[i], batch_cleaned[i]), f'frame {i} depends on what frame 1 holds'
    assert not torch.equal(batch[0], batch[2])
