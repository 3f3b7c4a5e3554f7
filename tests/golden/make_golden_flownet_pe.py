"""Generate golden_flownet_pe.npz FROM THE REFERENCE'S OWN CODE (the positional-encoding flow-field networks PEModel / PPEModel of
video-interpolation/model.py and LinearControllerEarly of video-interpolation/progressive_controller.py).

Run once where a checkout of the reference project is at hand (CPU only; the tests never need it):
    python tests/golden/make_golden_flownet_pe.py <reference checkout>/video-interpolation
Imports model.py and progressive_controller.py unmodified (torch + numpy only, CPU).  As in make_golden_flownet_grid.py the five
lines of FlowTrainer.forward (trainer.py:38-45) are applied to the imported model here, and a wrapped network is called as
main.py:136-143 leaves it: `controller(poses)`.

PositionalEncoding.forward reshapes through `.view(-1, 21)` and raises unless the number of points is a multiple of 7, so the grid
is t = 2 (times 0, 0.5), h = 21, w = 28: 1176 = 7 * 168 points (18 tiles of 64 and one of 24 rows).  scale = 3.  For PE and PPE,
each built with ModelParams() under torch.manual_seed(SEED[name]):
    {n}_keys, {n}_buf_{key}, {n}_head_{key} / {n}_tail_{key} / {n}_sum_{key}     as in make_golden_flownet.py
    encoding                          PositionalEncoding(3, 4) on the fp32 poses: (1176, 24) fp32
    PE_out32 / PE_out64               FlowTrainer.forward in fp32, and widened to float64
    PPE_out32_{k} / PPE_out64_{k}     k = ones: the bare network (no controller, no mask); ramp / mid: under `mask_{k}`, the masks of
                                      LinearControllerEarly(net, 1000, epsilon=1e-3) after 60 and 400 stash_iteration calls (loss 0.5):
                                      six ones and a block at 0.48, 15 closed; 18 ones, 9 closed
    {n}_gsum_{key} / {n}_gabs_{key} / {n}_gsub_{key}   float64 gradient of sum(flows64 * up) (PPE: under `mask_ramp`) for every
                                      parameter: sum, sum of magnitudes, every STRIDE-th element in flat order (all elements of
                                      biases, of the first and of the last layer)
    mask_ramp, mask_mid, mask_final   mask_final after all 1000 calls (all ones)
    trace                             (1000, 2) int64: (cur_block, next_block) after every stash_iteration call
    block_iterations, progress_iterations, block_size
    up
Outputs are data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = {'PE': 909, 'PPE': 1010}
TIMES, GH, GW, SCALE, STRIDE = (0.0, 0.5), 21, 28, 3.0, 97
MAX_ITERATION, EPSILON, N_RAMP, N_MID = 1000, 1e-3, 60, 400


def poses_of(T, dtype):
    H = torch.linspace(-1, 1, GH).to(dtype)                 # linspace is made in fp32 first, as the trainer does
    W = torch.linspace(-1, 1, GW).to(dtype)
    gridT, gridH, gridW = torch.meshgrid(T.to(dtype), H, W, indexing='ij')
    return torch.stack((gridT, gridH, gridW), dim=-1).view(-1, 3)


def shape_out(out):
    return out.view(len(TIMES), GH, GW, 4).permute(0, 3, 1, 2) * SCALE


def main():
    assert len(sys.argv) == 2, __doc__
    sys.path.insert(0, sys.argv[1])
    import model as ref_model                               # noqa: E402
    import progressive_controller as ref_pc                 # noqa: E402
    sys.path.pop(0)
    out = {}
    up = torch.randn(len(TIMES), 4, GH, GW, generator=torch.Generator().manual_seed(7))
    out['up'] = up.numpy()
    T = torch.tensor(TIMES)
    for name, seed in SEED.items():
        torch.manual_seed(seed)
        net = ref_model.model_dict[name](ref_model.ModelParams())
        prog = net.is_progressive
        assert net.encoding_dim == (27 if prog else 24)
        sd = net.state_dict()
        out[f'{name}_keys'] = np.array(list(sd.keys()))
        params = dict(net.named_parameters())
        for key, v in sd.items():
            if key in params:
                flat = v.detach().reshape(-1)
                out[f'{name}_head_{key}'] = flat[:32].numpy().copy()
                out[f'{name}_tail_{key}'] = flat[-32:].numpy().copy()
                out[f'{name}_sum_{key}'] = np.float64(flat.double().sum().item())
            else:
                out[f'{name}_buf_{key}'] = v.numpy().copy()
        net64 = ref_model.model_dict[name](ref_model.ModelParams()).double()
        net64.load_state_dict({k: v.double() for k, v in sd.items()})
        if not prog:
            with torch.no_grad():
                out['encoding'] = net.encode(poses_of(T, torch.float32)).contiguous().numpy()
                out[f'{name}_out32'] = shape_out(net(poses_of(T, torch.float32))).contiguous().numpy()
            flows64 = shape_out(net64(poses_of(T, torch.float64)))
            out[f'{name}_out64'] = flows64.detach().contiguous().numpy()
        else:
            ctl = ref_pc.LinearControllerEarly(net, MAX_ITERATION, epsilon=EPSILON)
            out['block_iterations'] = np.int64(ctl.block_iterations)
            out['progress_iterations'] = np.int64(ctl.progress_iterations)
            out['block_size'] = np.int64(ctl.block_size)
            masks, trace = {}, []
            for i in range(MAX_ITERATION):
                ctl.stash_iteration(torch.tensor(0.5))
                trace.append((ctl.cur_block, ctl.next_block))
                if i + 1 == N_RAMP:
                    masks['ramp'] = ctl.mask.clone()
                if i + 1 == N_MID:
                    masks['mid'] = ctl.mask.clone()
            masks['final'] = ctl.mask.clone()
            out['trace'] = np.array(trace, dtype=np.int64)
            for k, m in masks.items():
                out[f'mask_{k}'] = m.numpy().copy()
            ctl64 = ref_pc.LinearControllerEarly(net64, MAX_ITERATION, epsilon=EPSILON)
            with torch.no_grad():
                out[f'{name}_out32_ones'] = shape_out(net(poses_of(T, torch.float32))).contiguous().numpy()
                out[f'{name}_out64_ones'] = shape_out(net64(poses_of(T, torch.float64))).contiguous().numpy()
                for k in ('mid', 'ramp'):
                    ctl.mask = masks[k].clone()
                    ctl64.mask = masks[k].clone()
                    out[f'{name}_out32_{k}'] = shape_out(ctl(poses_of(T, torch.float32))).contiguous().numpy()
                    out[f'{name}_out64_{k}'] = shape_out(ctl64(poses_of(T, torch.float64))).contiguous().numpy()
            ctl64.mask = masks['ramp'].clone()
            flows64 = shape_out(ctl64(poses_of(T, torch.float64)))
            assert np.array_equal(flows64.detach().contiguous().numpy(), out[f'{name}_out64_ramp'])
        (flows64 * up.double()).sum().backward()
        for key, p in net64.named_parameters():
            g = p.grad.reshape(-1)
            out[f'{name}_gsum_{key}'] = np.float64(g.sum().item())
            out[f'{name}_gabs_{key}'] = np.float64(g.abs().sum().item())
            out[f'{name}_gsub_{key}'] = (g if g.numel() <= 8192 else g[::STRIDE]).numpy().copy()
    path = os.path.join(HERE, 'golden_flownet_pe.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
