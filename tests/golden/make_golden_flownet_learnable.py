"""Generate golden_flownet_learnable.npz FROM THE REFERENCE'S OWN CODE (the flow-field networks with learnable Fourier frequencies,
RFFModel / PRFFModel of video-interpolation/model.py, and the controller of video-interpolation/progressive_controller.py).

Run once where a checkout of the reference project is at hand (CPU only; the tests never need it):
    python tests/golden/make_golden_flownet_learnable.py <reference checkout>/video-interpolation
Imports model.py and progressive_controller.py unmodified (torch + numpy only, CPU).  As in make_golden_flownet.py the five lines of
FlowTrainer.forward (trainer.py:38-45) are applied to the imported model here; PRFF under a mask is called as main.py:136-143 leaves
it, `controller(poses)`, with LinearControllerEarly(net, 1000, epsilon=1e-3) as in make_golden_flownet_progressive.py.

For RFF and PRFF, each built with ModelParams() under torch.manual_seed(SEED[name]):
    {n}_keys, {n}_pkeys                  the state_dict keys and the names of the parameters, both in order
    {n}_buf_{key}                        the buffers in full (encode.magnitudes)
    {n}_head_{key} / {n}_tail_{key} / {n}_sum_{key}    first / last 32 values (fp32) and the float64 sum of every parameter
    {n}_frequencies                      encode.frequencies in full, (3, 256) fp32
and for every CASE of the network (RFF: `plain`; PRFF: `ones`, the bare network; `init`, the controller's first mask of 6 open
features; `ramp`, its mask after 98 stash_iteration calls at loss 0.5, whose block in progress stands at 0.5):
    {n}_out32_{case} / {n}_out64_{case}  FlowTrainer.forward on the grid t = 2 (times 0, 0.5), h = 20, w = 28, scale = 3: the fp32 model, and
                                         the same model and coordinates widened to float64
    {n}_gsum_{case}_{key} / {n}_gabs_{case}_{key} / {n}_gsub_{case}_{key}    float64 gradient of sum(flows64 * up) for every parameter: sum,
                                         sum of magnitudes, every STRIDE-th element in flat order (all elements up to 1024)
    {n}_gfreq_{case}                     the float64 gradient of encode.frequencies in full, (3, 256)
    mask_init, mask_ramp, up
Outputs are data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = {'RFF': 707, 'PRFF': 808}
TIMES, GH, GW, SCALE, STRIDE = (0.0, 0.5), 20, 28, 3.0, 97
MAX_ITERATION, EPSILON, N_RAMP = 1000, 1e-3, 98


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
        sd = net.state_dict()
        out[f'{name}_keys'] = np.array(list(sd.keys()))
        params = dict(net.named_parameters())
        out[f'{name}_pkeys'] = np.array(list(params.keys()))
        for key, v in sd.items():
            if key in params:
                flat = v.detach().reshape(-1)
                out[f'{name}_head_{key}'] = flat[:32].numpy().copy()
                out[f'{name}_tail_{key}'] = flat[-32:].numpy().copy()
                out[f'{name}_sum_{key}'] = np.float64(flat.double().sum().item())
            else:
                out[f'{name}_buf_{key}'] = v.numpy().copy()
        out[f'{name}_frequencies'] = sd['encode.frequencies'].numpy().copy()
        net64 = ref_model.model_dict[name](ref_model.ModelParams()).double()
        net64.load_state_dict({k: v.double() for k, v in sd.items()})
        if name == 'RFF':
            cases = {'plain': (net, net64)}
        else:
            assert net.is_progressive and net.encoding_dim == 515
            ctl = ref_pc.LinearControllerEarly(net, MAX_ITERATION, epsilon=EPSILON)
            masks = {'init': ctl.mask.clone()}
            for i in range(N_RAMP):
                ctl.stash_iteration(torch.tensor(0.5))
            masks['ramp'] = ctl.mask.clone()
            cases = {'ones': (net, net64)}
            for k, m in masks.items():
                out[f'mask_{k}'] = m.numpy().copy()
                c32 = ref_pc.LinearControllerEarly(net, MAX_ITERATION, epsilon=EPSILON)
                c64 = ref_pc.LinearControllerEarly(net64, MAX_ITERATION, epsilon=EPSILON)
                c32.mask, c64.mask = m.clone(), m.clone()
                cases[k] = (c32, c64)
        for case, (f32, f64) in cases.items():
            with torch.no_grad():
                out[f'{name}_out32_{case}'] = shape_out(f32(poses_of(T, torch.float32))).contiguous().numpy()
            net64.zero_grad()
            flows64 = shape_out(f64(poses_of(T, torch.float64)))
            out[f'{name}_out64_{case}'] = flows64.detach().contiguous().numpy()
            (flows64 * up.double()).sum().backward()
            for key, p in net64.named_parameters():
                g = p.grad.reshape(-1)
                out[f'{name}_gsum_{case}_{key}'] = np.float64(g.sum().item())
                out[f'{name}_gabs_{case}_{key}'] = np.float64(g.abs().sum().item())
                out[f'{name}_gsub_{case}_{key}'] = (g if g.numel() <= 1024 else g[::STRIDE]).numpy().copy()
            out[f'{name}_gfreq_{case}'] = net64.encode.frequencies.grad.numpy().copy()
            net64.zero_grad()
    path = os.path.join(HERE, 'golden_flownet_learnable.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
