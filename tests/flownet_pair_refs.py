"""The float64 restatement of the flow-field networks on TWO coordinates (ModelParams(domain_dim=2): one frame pair, poses (y, x)) in plain
torch: tests/test_flownet_pair_golden.py ties it to the reference's own model.py through its fixture, tests/test_gpu_flownet_pair.py measures
the kernels against it.  The encoders are those of tests/flownet_refs.py, which are written over the last axis of `poses` and of the buffers and
so evaluate the reference's two-term expressions on (N, 2) poses with centres (512, 2), frequencies (2, 256) and offsets (256, 2); what is
restated here is the call: a pose list instead of the (times, ys, xs) grid, as video-interpolation/pair_flow.py:55-59 makes it.
"""
import torch

from flownet_refs import layer1_input

NETS = ('RBF', 'FFN', 'UFF', 'RBFG', 'PRBF', 'PFF', 'PUFF', 'PRBFG')
PLAIN = NETS[:4]
PROGRESSIVE = NETS[4:]
SEED = {'RBF': 1201, 'FFN': 1202, 'UFF': 1203, 'RBFG': 1204, 'PRBF': 1205, 'PFF': 1206, 'PUFF': 1207, 'PRBFG': 1208}
PARAMS = dict(domain_dim=2, std_rbf=50, std=50)           # pair_flow.py:39


def build(name, seed=None):
    """the port's network `name` as pair_flow.py:39-40 builds it, under the fixture's seed"""
    from sin_inn_amd import flownet
    torch.manual_seed(SEED[name] if seed is None else seed)
    return flownet.flow_model_dict[name](flownet.ModelParams(**PARAMS))


def grid_poses(h, w, dtype=torch.float32, device='cpu'):
    """pair_flow.py:55-58: (h w, 2), columns (y, x); linspace is made in fp32 on the CPU first, as there"""
    ys, xs = torch.linspace(-1, 1, h).to(device=device, dtype=dtype), torch.linspace(-1, 1, w).to(device=device, dtype=dtype)
    gh, gw = torch.meshgrid(ys, xs, indexing='ij')
    return torch.stack((gh, gw), dim=-1).view(-1, 2)


def restate_at(name, bufs, weights, poses, scale, dtype, mask=None, gates=None):
    """net(poses) * scale in plain torch in `dtype`: (N, 2) -> (N, 4).  bufs / weights / mask / gates as flownet_refs.restate takes them; the
    mask of a progressive network has 514 values"""
    weights = [p.to(dtype) for p in weights]
    x = layer1_input(name, bufs, poses.to(dtype), mask)
    for l in range(3):
        pre = torch.nn.functional.linear(x, weights[2 * l], weights[2 * l + 1])
        x = torch.relu(pre) if gates is None else pre * gates[l].to(dtype)
    return torch.nn.functional.linear(x, weights[6], weights[7]) * scale


def reference_grads_at(name, bufs, weights, poses, scale, up, mask, gates):
    """{dtype: gradients of sum(out * up) with respect to the weights} of `restate_at` in float64 and in fp32; up (N, 4)"""
    out = {}
    for dtype in (torch.float64, torch.float32):
        w = [p.to(dtype).requires_grad_(True) for p in weights]
        flows = restate_at(name, bufs, w, poses, scale, dtype, mask, gates)
        out[dtype] = torch.autograd.grad((flows * up.to(dtype)).sum(), w)
    return out
