"""Generate golden_flownet_spatial.npz FROM THE REFERENCE'S OWN CODE (StashedSpatialController of
video-interpolation/progressive_controller.py around the progressive networks of video-interpolation/model.py).

Run once where a checkout of the reference project is at hand (CPU only; the tests never need it):
    python tests/golden/make_golden_flownet_spatial.py <reference checkout>/video-interpolation
Imports model.py and progressive_controller.py unmodified (torch + numpy only, CPU).

For n = PRBF (seed 404, res 4: 64 cells, k = 3) and PFF (seed 505, res 7: 343 cells, k = 5), each
StashedSpatialController(net, res, block_iterations=8, epsilon=1e-3):
    {n}_meta         res, k, block_size, block_iterations, progress_iterations
    {n}_keys         the keys of the controller's state dict
    {n}_stash_pts    points that share no corner cell (asserted here: torch's duplicate-index behaviour plays no part); {n}_stash_loss their
                     per-point loss: 1 where x > 0.6, else 1e-6
    {n}_mask_0 / _3 / _10   get_mask() of the fresh controller, after 3 and after 10 controller(points) + stash_iteration(loss) rounds
    {n}_mask_p       after the update_progress() that follows (it closes the cells whose blurred loss is below epsilon; the margin of every
                     cell to epsilon is asserted here to be wide, so rounding does not decide) and {n}_mask_p3 after 3 more rounds: the new
                     block ramps in the open cells only
    {n}_in_progress, {n}_cur_next   after update_progress
    {n}_sd_{key}     the state dict after that (not the model's entries)
    {n}_pts          about 200 points of [-1, 1]^3: the eight corners, points on cell boundaries, points just below one, random ones
    {n}_inds / {n}_alphas / {n}_interp   the stash and the interpolated mask of those points under the last state, {n}_out32 the network
                     output controller(points), {n}_out64 the same from a float64 copy of network and grid (cells and weights stay fp32)
Outputs are data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {'PRBF': (404, 4), 'PFF': (505, 7)}
BLOCK_ITERATIONS, EPSILON = 8, 1e-3


def stash_points(ctl, want, gen):
    """greedy: random points whose eight cells no earlier point touches"""
    taken, pts = set(), []
    for _ in range(4000):
        p = torch.rand(1, 3, generator=gen) * 2 - 1
        ctl.interpolate(p)
        cells = set(ctl.stash[0].flatten().tolist())
        if len(cells) == 8 and not (cells & taken):
            taken |= cells
            pts.append(p)
        if len(pts) == want:
            break
    return torch.cat(pts)


def probe_points(res, gen):
    span = max(res - 2, 1)
    corners = torch.tensor([[a, b, c] for a in (-1., 1.) for b in (-1., 1.) for c in (-1., 1.)])
    edges = []
    for j in range(1, res - 1):
        xb = torch.tensor(2 * (j - 0.5) / span - 1, dtype=torch.float32)
        for d in range(3):
            for v in (xb, xb - 4e-7, torch.nextafter(xb, torch.tensor(-2.))):
                p = torch.rand(3, generator=gen) * 2 - 1
                p[d] = v
                edges.append(p)
    edges = torch.stack(edges)
    rand = torch.rand(200 - 8 - edges.shape[0], 3, generator=gen) * 2 - 1
    return torch.cat((corners, edges, rand))


def main():
    assert len(sys.argv) == 2, __doc__
    sys.path.insert(0, sys.argv[1])
    import model as ref_model                               # noqa: E402
    import progressive_controller as ref_pc                 # noqa: E402
    sys.path.pop(0)
    out = {}
    for name, (seed, res) in CASES.items():
        torch.manual_seed(seed)
        net = ref_model.model_dict[name](ref_model.ModelParams())
        ctl = ref_pc.StashedSpatialController(net, res, block_iterations=BLOCK_ITERATIONS, epsilon=EPSILON)
        gen = torch.Generator().manual_seed(seed + 1)
        out[f'{name}_meta'] = np.array([ctl.res, ctl.k, ctl.block_size, ctl.block_iterations, ctl.progress_iterations])
        spts = stash_points(ctl, 20 if res > 4 else 5, gen)
        ctl.interpolate(spts)
        flat = ctl.stash[0].flatten()
        assert flat.unique().numel() == flat.numel(), 'the stash points share a cell'
        loss = torch.where(spts[:, 2] > 0.6, torch.tensor(1.0), torch.tensor(1e-6))
        out[f'{name}_stash_pts'], out[f'{name}_stash_loss'] = spts.numpy().copy(), loss.numpy().copy()
        out[f'{name}_mask_0'] = ctl.get_mask().numpy().copy()

        def rounds(n):
            for _ in range(n):
                with torch.no_grad():
                    ctl(spts)
                ctl.stash_iteration(loss)

        rounds(3)
        out[f'{name}_mask_3'] = ctl.get_mask().numpy().copy()
        rounds(7)
        out[f'{name}_mask_10'] = ctl.get_mask().numpy().copy()
        empty = ctl.not_visited_mask.clone()
        counter = ctl.log_counter.clone()
        counter[empty] = 1
        blurred = ctl.convolove_log((ctl.log_buffer / counter).clone(), empty)
        margin = float(((blurred - EPSILON).abs() / EPSILON).min())
        assert margin > 0.05, margin
        ctl.update_progress()
        closed = int((~ctl.in_progress).sum())
        assert 0 < closed < ctl.in_progress.numel(), closed
        print(name, 'res', res, 'k', ctl.k, 'stash points', spts.shape[0], 'closed cells', closed, '/', ctl.in_progress.numel(),
              'margin to epsilon', margin)
        out[f'{name}_mask_p'] = ctl.get_mask().numpy().copy()
        out[f'{name}_in_progress'] = ctl.in_progress.numpy().copy()
        out[f'{name}_cur_next'] = np.array([ctl.cur_block, ctl.next_block])
        sd = ctl.state_dict()
        out[f'{name}_keys'] = np.array(list(sd.keys()))
        for key, v in sd.items():
            if not key.startswith('model.'):
                out[f'{name}_sd_{key}'] = v.numpy().copy()
        rounds(3)
        out[f'{name}_mask_p3'] = ctl.get_mask().numpy().copy()

        pts = probe_points(res, gen)
        with torch.no_grad():
            o32, interp = ctl(pts, get_mask=True)
        out[f'{name}_pts'] = pts.numpy().copy()
        out[f'{name}_inds'], out[f'{name}_alphas'] = ctl.stash[0].numpy().copy(), ctl.stash[1].numpy().copy()
        out[f'{name}_interp'], out[f'{name}_out32'] = interp.numpy().copy(), o32.numpy().copy()
        net64 = ref_model.model_dict[name](ref_model.ModelParams()).double()
        net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
        with torch.no_grad():
            m64 = torch.einsum('ndf,nd->nf', ctl.get_mask().double()[ctl.stash[0]], ctl.stash[1].double())
            out[f'{name}_out64'] = net64(pts.double(), override_mask=m64).numpy().copy()
    path = os.path.join(HERE, 'golden_flownet_spatial.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
