"""Generate golden_flownet_piecewise.npz FROM THE REFERENCE'S OWN CODE (the piecewise-linear progressive flow-field network MPFFModel /
UniformPieceWiseEncoding of video-interpolation/model.py and LinearControllerEarly of video-interpolation/progressive_controller.py).

Run once where a checkout of the reference project is at hand (CPU only; the tests never need it):
    python tests/golden/make_golden_flownet_piecewise.py <reference checkout>/video-interpolation
Imports model.py and progressive_controller.py unmodified (torch + numpy only, CPU).  As in make_golden_flownet_grid.py the five lines of
FlowTrainer.forward (trainer.py:38-45) are applied to the imported model here, and a wrapped network is called as main.py:136-143 leaves
it: `controller(poses)`.  The reference's model_dict has no entry for this network; the class is taken by its name.

MPFFModel(ModelParams()) under torch.manual_seed(SEED), on the grid t = 2 (times 0, 0.5), h = 20, w = 28, scale = 3:
    MPFF_keys, MPFF_buf_{key}, MPFF_head_{key} / MPFF_tail_{key} / MPFF_sum_{key}     as in make_golden_flownet.py
    MPFF_out32_ones / MPFF_out64_ones   the bare network (no controller, no mask: all ones), fp32 and float64
    MPFF_out32_mid / MPFF_out64_mid     under `mask_mid`, the mask of LinearControllerEarly(net, 1000, epsilon=1e-3) after 100
                                        stash_iteration calls (loss 0.5)
    MPFF_out64_ramp                     float64 under `mask_ramp`, the mask after 98 calls: the block in progress stands at 0.5
    MPFF_gsum_{key} / MPFF_gabs_{key} / MPFF_gsub_{key}   float64 gradient of sum(flows64 * up) under `mask_ramp` for every parameter: sum,
                                        sum of magnitudes, every STRIDE-th element in flat order (all elements of biases and of the last
                                        layer)
    MPFF_gcoord                         the three coordinate columns of that gradient of the first weight, in full: (256, 3)
    MPFF_enc64_out                      the float64 encoding itself at 64 points of [-1.5, 1.5]^3 (`enc_poses`, seeded): (64, 512), the
                                        reference's values where u < 0 included
    mask_mid, mask_ramp, up, enc_poses
Outputs are data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAME, SEED = 'MPFF', 1414
TIMES, GH, GW, SCALE, STRIDE = (0.0, 0.5), 20, 28, 3.0, 97
MAX_ITERATION, EPSILON, N_RAMP, N_MID = 1000, 1e-3, 98, 100


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
    name = NAME
    torch.manual_seed(SEED)
    net = ref_model.MPFFModel(ref_model.ModelParams())
    assert net.is_progressive and net.encoding_dim == 515
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
    net64 = ref_model.MPFFModel(ref_model.ModelParams()).double()
    net64.load_state_dict({k: v.double() for k, v in sd.items()})
    ctl = ref_pc.LinearControllerEarly(net, MAX_ITERATION, epsilon=EPSILON)
    masks = {}
    for i in range(N_MID):
        ctl.stash_iteration(torch.tensor(0.5))
        if i + 1 == N_RAMP:
            masks['ramp'] = ctl.mask.clone()
    masks['mid'] = ctl.mask.clone()
    for k, m in masks.items():
        out[f'mask_{k}'] = m.numpy().copy()
    ctl64 = ref_pc.LinearControllerEarly(net64, MAX_ITERATION, epsilon=EPSILON)
    with torch.no_grad():
        out[f'{name}_out32_mid'] = shape_out(ctl(poses_of(T, torch.float32))).contiguous().numpy()
        out[f'{name}_out32_ones'] = shape_out(net(poses_of(T, torch.float32))).contiguous().numpy()
        ctl64.mask = masks['mid'].clone()
        out[f'{name}_out64_mid'] = shape_out(ctl64(poses_of(T, torch.float64))).contiguous().numpy()
        out[f'{name}_out64_ones'] = shape_out(net64(poses_of(T, torch.float64))).contiguous().numpy()
        enc_poses = torch.rand(64, 3, generator=torch.Generator().manual_seed(8)) * 3 - 1.5
        out['enc_poses'] = enc_poses.numpy().copy()
        out[f'{name}_enc64_out'] = net64.encode(enc_poses.double()).numpy().copy()
    ctl64.mask = masks['ramp'].clone()
    flows64 = shape_out(ctl64(poses_of(T, torch.float64)))
    out[f'{name}_out64_ramp'] = flows64.detach().contiguous().numpy()
    (flows64 * up.double()).sum().backward()
    for key, p in net64.named_parameters():
        g = p.grad.reshape(-1)
        out[f'{name}_gsum_{key}'] = np.float64(g.sum().item())
        out[f'{name}_gabs_{key}'] = np.float64(g.abs().sum().item())
        out[f'{name}_gsub_{key}'] = (g if g.numel() <= 1024 else g[::STRIDE]).numpy().copy()
    out[f'{name}_gcoord'] = net64.model.model[0].weight.grad[:, :3].numpy().copy()
    path = os.path.join(HERE, 'golden_flownet_piecewise.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
