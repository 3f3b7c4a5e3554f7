"""Generate golden_flownet.npz FROM THE REFERENCE'S OWN CODE (the flow-field networks of video-interpolation/model.py).

Run once where a checkout of the reference project is at hand (CPU only; the tests never need it):
    python tests/golden/make_golden_flownet.py <reference checkout>/video-interpolation
Imports video-interpolation/model.py unmodified (torch + numpy only, CPU).  trainer.py itself needs pytorch_lightning / apex and
is not imported: the five lines of FlowTrainer.forward (trainer.py:38-45) are applied to the imported model here.
For RBF, FFN and UFF, each built with ModelParams() under torch.manual_seed(SEED[name]):
    {n}_buf_{key}        the encoding buffers in full (fp32)
    {n}_keys             the state_dict keys, in order
    {n}_head_{key} / {n}_tail_{key} / {n}_sum_{key}   first / last 32 values (fp32) and the float64 sum of every parameter
                         (the 1 MB of weights is regenerated from the seed by the test)
    {n}_out32 / {n}_out64   FlowTrainer.forward on the grid t = 2 (times 0, 0.5), h = 20, w = 28, scale = 3: the fp32 model, and
                         the same model and coordinates widened to float64
    {n}_gsum_{key} / {n}_gabs_{key} / {n}_gsub_{key}  float64 gradient of sum(flows64 * up) for every parameter: its sum, its sum
                         of magnitudes and every STRIDE-th element of it in flat order (all elements for biases and the last layer;
                         the full float64 gradients of three models are 6 MB and do not belong in git)
    up                   the upstream gradient (2, 4, 20, 28), fp32
Outputs are data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = {'RBF': 101, 'FFN': 202, 'UFF': 303}
TIMES, GH, GW, SCALE, STRIDE = (0.0, 0.5), 20, 28, 3.0, 97


def trainer_forward(net, T, h, w, scale):
    H = torch.linspace(-1, 1, h).to(T)
    W = torch.linspace(-1, 1, w).to(T)
    gridT, gridH, gridW = torch.meshgrid(T, H, W, indexing='ij')
    poses = torch.stack((gridT, gridH, gridW), dim=-1).view(-1, 3)
    return net(poses).view(T.size(0), h, w, 4).permute(0, 3, 1, 2) * scale


def main():
    assert len(sys.argv) == 2, __doc__
    sys.path.insert(0, sys.argv[1])
    import model as ref_model                      # noqa: E402
    sys.path.pop(0)
    out = {}
    up = torch.randn(len(TIMES), 4, GH, GW, generator=torch.Generator().manual_seed(7))
    out['up'] = up.numpy()
    for name, seed in SEED.items():
        torch.manual_seed(seed)
        net = ref_model.model_dict[name](ref_model.ModelParams())
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
        T = torch.tensor(TIMES)
        with torch.no_grad():
            out[f'{name}_out32'] = trainer_forward(net, T, GH, GW, SCALE).contiguous().numpy()
        # float64: the same weights, buffers and fp32 coordinates, widened (linspace is made in fp32 first, as the trainer does)
        net64 = ref_model.model_dict[name](ref_model.ModelParams()).double()
        net64.load_state_dict({k: v.double() for k, v in sd.items()})

        def fwd64():
            H = torch.linspace(-1, 1, GH).double()
            W = torch.linspace(-1, 1, GW).double()
            gridT, gridH, gridW = torch.meshgrid(T.double(), H, W, indexing='ij')
            poses = torch.stack((gridT, gridH, gridW), dim=-1).view(-1, 3)
            return net64(poses).view(len(TIMES), GH, GW, 4).permute(0, 3, 1, 2) * SCALE
        flows64 = fwd64()
        out[f'{name}_out64'] = flows64.detach().contiguous().numpy()
        (flows64 * up.double()).sum().backward()
        for key, p in net64.named_parameters():
            g = p.grad.reshape(-1)
            out[f'{name}_gsum_{key}'] = np.float64(g.sum().item())
            out[f'{name}_gabs_{key}'] = np.float64(g.abs().sum().item())
            out[f'{name}_gsub_{key}'] = (g if g.numel() <= 1024 else g[::STRIDE]).numpy().copy()
    path = os.path.join(HERE, 'golden_flownet.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
