"""Generate golden_flowtrainer.npz FROM THE REFERENCE'S OWN CODE (flow visualisation and .flo IO of the flow trainer).

Run once in the build container (needs /root/reference; never runs on the GPU box):
    python tests/golden/make_golden_flowtrainer.py
Imports video-interpolation/my_utils/flow_viz.py and my_utils/utils.py unmodified (pure numpy / torch, CPU).  Outputs are data
only: inputs and expected outputs.

flow2img cases (inputs `f2i_<case>_flow` (2, h, w) fp32, `f2i_<case>_clip`, outputs `f2i_<case>_img` (3, h, w) uint8):
    random      13 x 37, sigma 4: some values go past the default clip of 10
    clip50      the same flow with clip=50
    zero        all zero: maxrad == 0, every pixel NaN, every pixel black
    unknown     a value above 1e7 (clipped before the unknown-flow test ever sees it) and a NaN (rad.max() is NaN, and Python's
                max(-1, nan) makes maxrad -1)
    radial      a fan around the centre that sweeps every colour-wheel sector, radius up to 1.5 x clip: both branches of rad <= 1
.flo: `flo_field` (5, 7, 2) fp32, `flo_bytes` the file writeFlow produces for it, `flo_read` what readFlow returns for that file.
"""
import os
import sys
import tempfile

import numpy as np
import torch

REF = '/root/reference/video-interpolation'
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 31


def main():
    sys.path.insert(0, os.path.join(REF, 'my_utils'))
    import flow_viz as ref_viz          # noqa: E402
    import utils as ref_utils           # noqa: E402
    sys.path.pop(0)
    g = torch.Generator().manual_seed(SEED)
    out = {}
    rnd = torch.randn(2, 13, 37, generator=g) * 4
    unknown = torch.randn(2, 13, 37, generator=g) * 4
    unknown[0, 3, 5] = 3e7
    unknown[1, 8, 30] = float('nan')
    yy, xx = torch.meshgrid(torch.arange(41, dtype=torch.float32) - 20, torch.arange(59, dtype=torch.float32) - 29, indexing='ij')
    radial = torch.stack((xx, yy)) * (15.0 / 29.0)
    cases = {'random': (rnd, 10), 'clip50': (rnd, 50), 'zero': (torch.zeros(2, 13, 37), 10), 'unknown': (unknown, 10),
             'radial': (radial, 10)}
    with np.errstate(all='ignore'):
        for name, (flow, clip) in cases.items():
            img = ref_viz.flow2img(flow.clone(), clip=clip)
            assert img.dtype == torch.uint8 and tuple(img.shape) == (3,) + tuple(flow.shape[1:])
            out[f'f2i_{name}_flow'] = flow.numpy()
            out[f'f2i_{name}_clip'] = np.array(clip, np.float32)
            out[f'f2i_{name}_img'] = img.numpy()
    field = (torch.randn(5, 7, 2, generator=g) * 3).numpy()
    with tempfile.TemporaryDirectory() as tmp:
        fn = os.path.join(tmp, 'field.flo')
        ref_utils.writeFlow(fn, field)
        out['flo_field'] = field
        out['flo_bytes'] = np.frombuffer(open(fn, 'rb').read(), np.uint8)
        out['flo_read'] = ref_utils.readFlow(fn)
    np.savez_compressed(os.path.join(HERE, 'golden_flowtrainer.npz'), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
