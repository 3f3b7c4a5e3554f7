"""Generate golden_flownet_progressive.npz FROM THE REFERENCE'S OWN CODE (the progressive flow-field networks of
video-interpolation/model.py and the controllers of video-interpolation/progressive_controller.py).

Run once where a checkout of the reference project is at hand (CPU only; the tests never need it):
    python tests/golden/make_golden_flownet_progressive.py <reference checkout>/video-interpolation
Imports model.py and progressive_controller.py unmodified (torch + numpy only, CPU).  As in make_golden_flownet.py the five lines of
FlowTrainer.forward (trainer.py:38-45) are applied to the imported model here; a wrapped network is called as main.py:136-143 leaves
it: `controller(poses)`, which multiplies the 515 features by the controller's mask.

For PRBF, PFF and PUFF, each built with ModelParams() under torch.manual_seed(SEED[name]) and wrapped in
LinearControllerEarly(net, 1000, epsilon=1e-3):
    {n}_keys, {n}_buf_{key}, {n}_head_{key} / {n}_tail_{key} / {n}_sum_{key}     as in make_golden_flownet.py
    {n}_out32_mid / {n}_out64_mid     FlowTrainer.forward on the grid t = 2 (times 0, 0.5), h = 20, w = 28, scale = 3 under `mask_mid`,
                                      the controller's mask after 100 stash_iteration calls (loss 0.5): fp32, and widened to float64
    {n}_out32_ones / {n}_out64_ones   the bare network (no controller, no mask: all ones)
    {n}_out64_ramp                    float64 under `mask_ramp`, the mask after 98 calls: the block in progress stands at 0.5
    {n}_gsum_{key} / {n}_gabs_{key} / {n}_gsub_{key}   float64 gradient of sum(flows64 * up) under `mask_ramp` for every parameter: sum,
                                      sum of magnitudes, every STRIDE-th element in flat order (all elements of biases and of the last layer)
    {n}_gcoord                        the three coordinate columns of that gradient of the first weight, in full: (256, 3)
    mask_mid, mask_ramp, mask_init, up
Controller trajectory, on the PRBF network, max_iteration = 1000, scripted loss 0.5 for 300 iterations and 5e-4 after, for
LinearController (`lin`) and LinearControllerEarly(epsilon=1e-3) (`early`), at the iterations ITERS:
    traj_{c}_mask (len(ITERS), 515), traj_{c}_cur, traj_{c}_next, traj_{c}_stashed (mask_stashed of state_dict() at that iteration)
    rt_{c}_ramp_saved / rt_{c}_ramp_loaded     the mask at iteration 98 and the mask a fresh controller holds after load_state_dict of that
                                               state (they differ: six entries at 0.5 come back as three ones)
    rt_{c}_final_saved / rt_{c}_final_loaded   the same at iteration 1000 (equal)
    traj_meta   block_size, block_iterations, progress_iterations
Outputs are data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = {'PRBF': 404, 'PFF': 505, 'PUFF': 606}
TIMES, GH, GW, SCALE, STRIDE = (0.0, 0.5), 20, 28, 3.0, 97
MAX_ITERATION, EPSILON, N_RAMP, N_MID = 1000, 1e-3, 98, 100
ITERS = (1, 2, 3, 4, 7, 8, 9, 12, 16, 97, 98, 100, 299, 300, 301, 302, 500, 671, 672, 673, 1000)


def poses_of(T, dtype):
    H = torch.linspace(-1, 1, GH).to(dtype)                 # linspace is made in fp32 first, as the trainer does
    W = torch.linspace(-1, 1, GW).to(dtype)
    gridT, gridH, gridW = torch.meshgrid(T.to(dtype), H, W, indexing='ij')
    return torch.stack((gridT, gridH, gridW), dim=-1).view(-1, 3)


def shape_out(out):
    return out.view(len(TIMES), GH, GW, 4).permute(0, 3, 1, 2) * SCALE


def scripted_loss(i):
    return torch.tensor(0.5 if i < 300 else 5e-4)


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
        ctl = ref_pc.LinearControllerEarly(net, MAX_ITERATION, epsilon=EPSILON)
        masks = {'init': ctl.mask.clone()}
        for i in range(N_MID):
            ctl.stash_iteration(scripted_loss(i))
            if i + 1 == N_RAMP:
                masks['ramp'] = ctl.mask.clone()
        masks['mid'] = ctl.mask.clone()
        for k, m in masks.items():
            if f'mask_{k}' in out:
                assert np.array_equal(out[f'mask_{k}'], m.numpy())
            out[f'mask_{k}'] = m.numpy().copy()
        net64 = ref_model.model_dict[name](ref_model.ModelParams()).double()
        net64.load_state_dict({k: v.double() for k, v in sd.items()})
        ctl64 = ref_pc.LinearControllerEarly(net64, MAX_ITERATION, epsilon=EPSILON)
        with torch.no_grad():
            out[f'{name}_out32_mid'] = shape_out(ctl(poses_of(T, torch.float32))).contiguous().numpy()
            out[f'{name}_out32_ones'] = shape_out(net(poses_of(T, torch.float32))).contiguous().numpy()
            ctl64.mask = masks['mid'].clone()
            out[f'{name}_out64_mid'] = shape_out(ctl64(poses_of(T, torch.float64))).contiguous().numpy()
            out[f'{name}_out64_ones'] = shape_out(net64(poses_of(T, torch.float64))).contiguous().numpy()
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

    def fresh(kind):
        torch.manual_seed(SEED['PRBF'])
        net = ref_model.model_dict['PRBF'](ref_model.ModelParams())
        if kind == 'lin':
            return ref_pc.LinearController(net, MAX_ITERATION)
        return ref_pc.LinearControllerEarly(net, MAX_ITERATION, epsilon=EPSILON)

    for kind in ('lin', 'early'):
        ctl = fresh(kind)
        out['traj_meta'] = np.array([ctl.block_size, ctl.block_iterations, ctl.progress_iterations])
        rec = {k: [] for k in ('mask', 'cur', 'next', 'stashed')}
        for i in range(MAX_ITERATION):
            ctl.stash_iteration(scripted_loss(i))
            it = i + 1
            if it in ITERS:
                state = ctl.state_dict()
                rec['mask'].append(ctl.mask.numpy().copy())
                rec['cur'].append(ctl.cur_block)
                rec['next'].append(ctl.next_block)
                rec['stashed'].append(state['mask_stashed'].numpy().copy())
            if it in (N_RAMP, MAX_ITERATION):
                tag = 'ramp' if it == N_RAMP else 'final'
                other = fresh(kind)
                other.load_state_dict({k: v.clone() for k, v in ctl.state_dict().items()})
                out[f'rt_{kind}_{tag}_saved'] = ctl.mask.numpy().copy()
                out[f'rt_{kind}_{tag}_loaded'] = other.mask.numpy().copy()
        out[f'traj_{kind}_mask'] = np.stack(rec['mask'])
        out[f'traj_{kind}_cur'] = np.array(rec['cur'])
        out[f'traj_{kind}_next'] = np.array(rec['next'])
        out[f'traj_{kind}_stashed'] = np.stack(rec['stashed'])
        print(kind, 'ends at', ctl.cur_block, '/', ctl.encoding_dim, 'mask sum', float(ctl.mask.sum()))
    path = os.path.join(HERE, 'golden_flownet_progressive.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
