"""Generate golden_flownet_pair.npz FROM THE REFERENCE'S OWN CODE: the flow-field networks of video-interpolation/model.py built the way
video-interpolation/pair_flow.py:39-42 builds its one, ModelParams(domain_dim=2, std_rbf=50, std=50), and LinearControllerEarly of
video-interpolation/progressive_controller.py around the progressive ones.

Run once where a checkout of the reference project is at hand (CPU only; the tests never need it):
    python tests/golden/make_golden_flownet_pair.py <reference checkout>/video-interpolation
Imports model.py and progressive_controller.py unmodified (torch + numpy only, CPU).  A network is called as pair_flow.py:59 calls it,
`net(poses)` on a pose list (N, 2), columns (y, x); a wrapped one as `controller(poses)`.

For RBF, FFN, UFF, RBFG, PRBF, PFF, PUFF and PRBFG, each built under torch.manual_seed(SEED[name]), at `poses`, 37 points (the first four
the corners of [-1, 1]^2, the rest uniform from a seeded generator):
    {n}_keys, {n}_shapes                 the state dict's keys and the shape of every entry (rows padded with -1)
    {n}_buf_{key}                        every encoder buffer, in full
    {n}_out32 / {n}_out64                net(poses) in fp32, and widened to float64 (progressive: the bare network, no mask)
    {n}_out32_mid / {n}_out64_mid        progressive: under `mask_mid`
    {n}_out64_ramp                       progressive: float64 under `mask_ramp`
    mask_init, mask_ramp, mask_mid       the mask of LinearControllerEarly(PRBF, 1000, epsilon=1e-3) as built, after 97 (the block in progress stands at 0.8) and after 100
                                         stash_iteration calls (loss 0.5): 514 values, blocks of 4
    traj_meta, traj_mask, traj_cur, traj_next   block_size / block_iterations / progress_iterations, and the mask, cur_block and
                                         next_block after the ITERS-th call of a scripted run (loss 0.5, from call 300 on 5e-4)
No hidden-layer weights are stored: the constructors of the port reproduce them from the seed.  Outputs are data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = {'RBF': 1201, 'FFN': 1202, 'UFF': 1203, 'RBFG': 1204, 'PRBF': 1205, 'PFF': 1206, 'PUFF': 1207, 'PRBFG': 1208}
PARAMS = dict(domain_dim=2, std_rbf=50, std=50)
N_POSES, POSE_SEED = 37, 1200
MAX_ITERATION, EPSILON, N_RAMP, N_MID = 1000, 1e-3, 97, 100
ITERS = (1, 2, 3, 4, 5, 6, 97, 98, 100, 299, 300, 301, 500, 1000)


def make_poses():
    corners = torch.tensor([[-1.0, -1.0], [-1.0, 1.0], [1.0, -1.0], [1.0, 1.0]])
    rest = torch.rand(N_POSES - 4, 2, generator=torch.Generator().manual_seed(POSE_SEED)) * 2 - 1
    return torch.cat((corners, rest))


def main():
    assert len(sys.argv) == 2, __doc__
    sys.path.insert(0, sys.argv[1])
    import model as ref_model                               # noqa: E402
    import progressive_controller as ref_pc                 # noqa: E402
    sys.path.pop(0)
    out = {}
    poses = make_poses()
    out['poses'] = poses.numpy().copy()
    out['seeds'] = np.array([SEED[n] for n in SEED])
    out['names'] = np.array(list(SEED))
    for name, seed in SEED.items():
        torch.manual_seed(seed)
        net = ref_model.model_dict[name](ref_model.ModelParams(**PARAMS))
        prog = net.is_progressive
        assert net.encoding_dim == (514 if prog else 512)
        sd = net.state_dict()
        out[f'{name}_keys'] = np.array(list(sd.keys()))
        shapes = -np.ones((len(sd), 2), np.int64)
        params = dict(net.named_parameters())
        for i, (key, v) in enumerate(sd.items()):
            shapes[i, :v.dim()] = list(v.shape)
            if key not in params:
                out[f'{name}_buf_{key}'] = v.numpy().copy()
        out[f'{name}_shapes'] = shapes
        net64 = ref_model.model_dict[name](ref_model.ModelParams(**PARAMS)).double()
        net64.load_state_dict({k: v.double() for k, v in sd.items()})
        with torch.no_grad():
            out[f'{name}_out32'] = net(poses).numpy().copy()
            out[f'{name}_out64'] = net64(poses.double()).numpy().copy()
        if not prog:
            continue
        ctl = ref_pc.LinearControllerEarly(net, MAX_ITERATION, epsilon=EPSILON)
        if name == 'PRBF':
            out['mask_init'] = ctl.mask.numpy().copy()
            out['traj_meta'] = np.array([ctl.block_size, ctl.block_iterations, ctl.progress_iterations])
        masks = {}
        for i in range(N_MID):
            ctl.stash_iteration(torch.tensor(0.5))
            if i + 1 == N_RAMP:
                masks['ramp'] = ctl.mask.clone()
        masks['mid'] = ctl.mask.clone()
        if name == 'PRBF':
            for k, m in masks.items():
                out[f'mask_{k}'] = m.numpy().copy()
        ctl64 = ref_pc.LinearControllerEarly(net64, MAX_ITERATION, epsilon=EPSILON)
        with torch.no_grad():
            out[f'{name}_out32_mid'] = ctl(poses).numpy().copy()
            ctl64.mask = masks['mid'].clone()
            out[f'{name}_out64_mid'] = ctl64(poses.double()).numpy().copy()
            ctl64.mask = masks['ramp'].clone()
            out[f'{name}_out64_ramp'] = ctl64(poses.double()).numpy().copy()
        if name == 'PRBF':
            torch.manual_seed(seed)
            ctl = ref_pc.LinearControllerEarly(ref_model.model_dict[name](ref_model.ModelParams(**PARAMS)), MAX_ITERATION, epsilon=EPSILON)
            tm, tc, tn = [], [], []
            for i in range(MAX_ITERATION):
                ctl.stash_iteration(torch.tensor(0.5 if i < 300 else 5e-4))
                if i + 1 in ITERS:
                    tm.append(ctl.mask.numpy().copy())
                    tc.append(ctl.cur_block)
                    tn.append(ctl.next_block)
            out['traj_mask'], out['traj_cur'], out['traj_next'] = np.stack(tm), np.array(tc), np.array(tn)
    path = os.path.join(HERE, 'golden_flownet_pair.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
