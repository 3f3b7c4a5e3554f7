"""Record what the Python and command-line layer of the flow networks accepts and refuses, before any device is touched.

    python tests/golden/make_golden_flownet_python_refusals.py          # writes tests/golden/flownet_python_refusals.json

`record()` is the matrix; tests/test_flowcaps_host.py replays it on the working tree and compares every entry exactly.  Every call runs on
a machine without a GPU: a refusal is recorded as its exception type and full message, a call that gets past the refusals ends at the
"runs on the GPU only" NotImplementedError of `flownet._on_gpu`, which is recorded the same way.  Three parts:

    flownet   for every network of flow_model_dict, with 3 and with 2 coordinates, bare and (progressive) under a LinearControllerEarly and a
              StashedSpatialController: flow_at with jacobian= (alone, with pose_grad, with get_mask, with a 2-D override_mask, with poses that
              require a gradient), _refuse_jacobian(what='--loss-smooth-at'), flow_fields, flow_at plain / pose_grad / 2-D override_mask
    cli       video-interpolation/main.py get_args: the sentence after `error: ` and the exit status, or the attributes the options set
    trainer   FlowTrainer.__init__ on a namespace built directly: the same option sets, and each range / choice the constructor checks
"""
import contextlib
import importlib.util
import io
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden', 'flownet_python_refusals.json')
OPTION_ATTRS = ('net', 'spatially_adaptive', 'loss_between', 'between_taus', 'between_back', 'between_points', 'loss_smooth_at',
                'smooth_points')
TRAINER_ATTRS = ('between_weight', 'between_taus', 'between_back', 'between_points', 'smooth_at_weight', 'smooth_points')


def outcome(fn, show=lambda r: 'returned'):
    try:
        return show(fn())
    except SystemExit as e:                                # argparse: the sentence after the program's name
        return f'exit {e.code}'
    except Exception as e:
        return f'{type(e).__name__}: {e}'


def flow_main():
    spec = importlib.util.spec_from_file_location('flow_main_refusals', os.path.join(ROOT, 'video-interpolation', 'main.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def wrappers(flownet, progressive, name, dim):
    """{how the network is held: a thunk that builds it}; the controllers only around a progressive network"""
    def net():
        return flownet.flow_model_dict[name](flownet.ModelParams(domain_dim=dim))
    held = {'bare': net}
    if flownet.flow_model_dict[name].is_progressive:
        held['LinearControllerEarly'] = lambda: progressive.LinearControllerEarly(net(), 1000)
        held['StashedSpatialController'] = lambda: progressive.StashedSpatialController(net(), 3)
    return held


def flownet_entries():
    import torch
    from sin_inn_amd import flownet, progressive
    entries = {}
    for name in flownet.flow_model_dict:
        for dim in (3, 2):
            for how, build in wrappers(flownet, progressive, name, dim).items():
                key = f'{name} dim {dim} {how}'
                try:
                    net = build()
                except Exception as e:
                    entries[f'{key}: construction'] = f'{type(e).__name__}: {e}'
                    continue
                poses = torch.zeros(5, dim)
                grid = torch.ones(27, net.encoding_dim)
                calls = {
                    "flow_at(jacobian='yx')": lambda: flownet.flow_at(net, poses, jacobian='yx'),
                    "flow_at(jacobian='yx', pose_grad=True)": lambda: flownet.flow_at(net, poses, jacobian='yx', pose_grad=True),
                    "flow_at(jacobian='yx', get_mask=True)": lambda: flownet.flow_at(net, poses, jacobian='yx', get_mask=True),
                    "flow_at(jacobian='yx', override_mask=2-D)": lambda: flownet.flow_at(net, poses, jacobian='yx', override_mask=grid),
                    "flow_at(jacobian='yx') poses.requires_grad": lambda: flownet.flow_at(net, poses.clone().requires_grad_(), jacobian='yx'),
                    "_refuse_jacobian(what='--loss-smooth-at')": lambda: flownet._refuse_jacobian(net, what='--loss-smooth-at'),
                    'flow_fields': lambda: flownet.flow_fields(net, torch.zeros(2) if dim == 3 else None, 4, 6, 1.0),
                    'flow_fields(override_mask=2-D)': lambda: flownet.flow_fields(net, torch.zeros(2) if dim == 3 else None, 4, 6, 1.0,
                                                                                  override_mask=grid),
                    'flow_fields times the other way': lambda: flownet.flow_fields(net, None if dim == 3 else torch.zeros(2), 4, 6, 1.0),
                    'flow_at': lambda: flownet.flow_at(net, poses),
                    'flow_at(pose_grad=True)': lambda: flownet.flow_at(net, poses, pose_grad=True),
                    'flow_at(override_mask=2-D)': lambda: flownet.flow_at(net, poses, override_mask=grid),
                    'flow_at poses of the other dimension': lambda: flownet.flow_at(net, torch.zeros(5, 5 - dim)),
                }
                for call, fn in calls.items():
                    entries[f'{key}: {call}'] = outcome(fn)
    return entries


def cli_cases(names):
    cases = []
    for name in names:
        for extra in ([], ['--spatially-adaptive'], ['--loss-smooth-at', '1'], ['--spatially-adaptive', '--loss-smooth-at', '1']):
            cases.append(['--net', name] + extra)
    for weights in ([], ['--loss-between', '1'], ['--loss-smooth-at', '1']):
        cases += [weights + ['--between-taus', '2', '--between-points', '8'], weights + ['--between-points', '0'],
                  weights + ['--between-points', '8'], weights + ['--between-taus', '0'], weights + ['--between-taus', '33'],
                  weights + ['--smooth-points', '0'], weights + ['--smooth-points', '8'], weights + ['--between-points', str(1 << 23)],
                  weights + ['--smooth-points', str(1 << 23)], weights + ['--between-back', 'reverse']]
    cases.append(['--between-back', 'sideways'])
    return cases


def cli_entries(names):
    m = flow_main()
    entries = {}
    for argv in cli_cases(names):
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            got = outcome(lambda: m.get_args(['train'] + argv),
                          lambda a: {k: getattr(a, k, '<absent>') for k in OPTION_ATTRS})
        if isinstance(got, str) and got.startswith('exit'):
            got += ': ' + err.getvalue().split('error: ', 1)[1].strip()
        entries[' '.join(argv)] = got
    return entries


def trainer_cases(names):
    """(label, network name, domain_dim, spatial controller?, the attributes set on the namespace)"""
    cases = []
    for name in names:
        cases += [(name, 3, False, {}), (name, 3, False, dict(loss_smooth_at=1.0)),
                  (name, 3, True, {}), (name, 3, True, dict(loss_smooth_at=1.0)), (name, 2, False, dict(loss_smooth_at=1.0))]
    on = dict(loss_between=1.0, between_dt=0.5)
    for opts in (dict(between_taus=2, between_points=8), dict(on, between_taus=2, between_points=8), dict(on, between_points=0),
                 dict(between_points=0), dict(on, between_points=8), dict(on, between_points=(1 << 22) + 1), dict(on, between_taus=0),
                 dict(on, between_taus=33), dict(on, between_taus=32), dict(on, between_back='sideways'), dict(on, between_back='reverse'),
                 dict(loss_between=1.0), dict(loss_between=1.0, between_dt=0.0), dict(on, between_taus=0, between_points=0),
                 dict(smooth_points=0), dict(loss_smooth_at=1.0, smooth_points=0), dict(loss_smooth_at=1.0, smooth_points=8),
                 dict(loss_smooth_at=1.0, smooth_points=-1), dict(loss_smooth_at=1.0, smooth_points=(1 << 22) + 1),
                 dict(on, loss_smooth_at=1.0, between_taus=0, smooth_points=-1)):
        cases.append(('RBF', 3, False, opts))
        cases.append(('PE', 3, False, opts))                # a network without the Jacobian: which refusal comes first
    cases.append(('RBF', 2, False, on))
    return cases


def trainer_entries(names):
    from sin_inn_amd import flownet, flowtrainer, progressive
    m = flow_main()
    entries = {}
    for name, dim, spatial, opts in trainer_cases(names):
        label = f"{name} dim {dim}{' spatial' if spatial else ''} {' '.join(f'{k}={v}' for k, v in opts.items())}".strip()
        if spatial and not flownet.flow_model_dict[name].is_progressive:
            continue
        args = m.get_args(['train'])
        net = flownet.flow_model_dict[name](flownet.ModelParams(domain_dim=dim))
        if spatial:
            net = progressive.StashedSpatialController(net, 3)
        elif net.is_progressive:
            net = progressive.LinearControllerEarly(net, 1000)
        args.net, args.spatially_adaptive = net, spatial
        for k, v in opts.items():
            setattr(args, k, v)
        entries[label] = outcome(lambda: flowtrainer.FlowTrainer(args), lambda t: {k: getattr(t, k, '<absent>') for k in TRAINER_ATTRS})
    return entries


def record():
    from sin_inn_amd import flownet
    names = list(flownet.flow_model_dict)
    return {'flownet': flownet_entries(), 'cli': cli_entries(names + ['bogus']), 'trainer': trainer_entries(names)}


if __name__ == '__main__':
    commit = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True, check=True).stdout.strip()
    doc = {'commit': commit,
           'how': 'tests/golden/make_golden_flownet_python_refusals.py record(), run at that commit on a machine without a GPU: the exception '
                  'type and full message of each call, or what it returned; a call past the refusals ends at the "runs on the GPU only" error',
           **record()}
    with open(OUT, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(OUT, {k: len(v) for k, v in doc.items() if isinstance(v, dict)})
