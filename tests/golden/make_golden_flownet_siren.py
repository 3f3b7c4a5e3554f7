"""Generate golden_flownet_siren.npz FROM THE REFERENCE'S OWN CODE (SirenModel / SineLayer of video-interpolation/model.py:123-171).

Run once where a checkout of the reference project is at hand (CPU only; the tests never need it):
    python tests/golden/make_golden_flownet_siren.py <reference checkout>/video-interpolation
Imports model.py unmodified (torch + numpy only, CPU).  As in make_golden_flownet_pe.py the five lines of FlowTrainer.forward
(trainer.py:38-45) are applied to the imported model here.

The grid is t = 2 (times 0, 0.5), h = 21, w = 28: 1176 points (18 tiles of 64 and one of 24 rows, a tile straddling the two frames).
scale = 3.  For `siren`, built with ModelParams() under torch.manual_seed(SEED):
    keys                              the state_dict keys in order
    head_{key} / tail_{key} / sum_{key}   first 32 and last 32 values (flat order) and the float64 sum of every parameter
    out32 / out64                     FlowTrainer.forward in fp32, and widened to float64
    up                                randn(2, 4, 21, 28), generator seed 7
    gsum_{key} / gabs_{key} / gsub_{key}   float64 gradient of sum(flows64 * up) for every parameter: sum, sum of magnitudes, every
                                      STRIDE-th element in flat order (all elements of biases, of the first and of the last layer)
Outputs are data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 1111
TIMES, GH, GW, SCALE, STRIDE = (0.0, 0.5), 21, 28, 3.0, 97


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
    sys.path.pop(0)
    out = {}
    up = torch.randn(len(TIMES), 4, GH, GW, generator=torch.Generator().manual_seed(7))
    out['up'] = up.numpy()
    T = torch.tensor(TIMES)
    torch.manual_seed(SEED)
    net = ref_model.model_dict['siren'](ref_model.ModelParams())
    assert not net.is_progressive and net.encoding_dim == 3
    sd = net.state_dict()
    out['keys'] = np.array(list(sd.keys()))
    for key, v in sd.items():
        flat = v.detach().reshape(-1)
        out[f'head_{key}'] = flat[:32].numpy().copy()
        out[f'tail_{key}'] = flat[-32:].numpy().copy()
        out[f'sum_{key}'] = np.float64(flat.double().sum().item())
    net64 = ref_model.model_dict['siren'](ref_model.ModelParams()).double()
    net64.load_state_dict({k: v.double() for k, v in sd.items()})
    with torch.no_grad():
        out['out32'] = shape_out(net(poses_of(T, torch.float32))).contiguous().numpy()
    flows64 = shape_out(net64(poses_of(T, torch.float64)))
    out['out64'] = flows64.detach().contiguous().numpy()
    (flows64 * up.double()).sum().backward()
    for key, p in net64.named_parameters():
        g = p.grad.reshape(-1)
        out[f'gsum_{key}'] = np.float64(g.sum().item())
        out[f'gabs_{key}'] = np.float64(g.abs().sum().item())
        out[f'gsub_{key}'] = (g if g.numel() <= 8192 else g[::STRIDE]).numpy().copy()
    path = os.path.join(HERE, 'golden_flownet_siren.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
