"""No GPU needed: the capability table of the flow networks (sin_inn_amd/flowcaps.py) and everything that reads it.

tests/golden/flownet_python_refusals.json was recorded at the commit it names, before the table existed, by
tests/golden/make_golden_flownet_python_refusals.py: what flow_at / flow_fields / _refuse_jacobian, main.py get_args and
FlowTrainer.__init__ accepted and refused, message for message, for every network.  The same matrix is replayed here and compared exactly.
"""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'flownet_python_refusals.json')


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def replay():
    return json.loads(json.dumps(_load('make_refusals', 'tests', 'golden', 'make_golden_flownet_python_refusals.py').record()))


@pytest.mark.parametrize('part', ['flownet', 'cli', 'trainer'])
def test_every_refusal_is_the_recorded_one(replay, part):
    with open(GOLDEN) as f:
        golden = json.load(f)[part]
    assert len(golden) > 90 and sorted(replay[part]) == sorted(golden)
    wrong = {k: (replay[part][k], v) for k, v in golden.items() if replay[part][k] != v}
    assert not wrong, f'{len(wrong)} of {len(golden)} differ, the first: {next(iter(wrong.items()))}'


def test_name_sets_are_the_literal_ones():
    from sin_inn_amd import flowcaps, flownet
    m = _load('flow_main_caps', 'video-interpolation', 'main.py')
    pair = _load('pair_flow_caps', 'video-interpolation', 'pair_flow.py')
    assert m.NETWORKS == ('RBF', 'FFN', 'UFF', 'PRBF', 'PFF', 'PUFF', 'RFF', 'PRFF', 'RBFG', 'PRBFG', 'PE', 'PPE')
    assert m.OUT_OF_SCOPE_NETWORKS == ('siren', 'MPFF')
    assert m.JACOBIAN_NETWORKS == ('RBF', 'FFN', 'UFF', 'PRBF', 'PFF', 'PUFF')
    assert m.SPATIAL_NETWORKS == ('PRBF', 'PFF', 'PUFF', 'PRFF', 'PRBFG')
    assert pair.NETWORKS == ('RBF', 'FFN', 'UFF', 'RBFG', 'PRBF', 'PFF', 'PUFF', 'PRBFG')
    assert m.NETWORKS == tuple(flownet.all_model_dict) and set(flowcaps.TABLE) == set(flownet.flow_model_dict)


def test_rows_describe_the_model_classes():
    """kind, progressive, learnable and the width of layer 1 are those of the module a name builds; a model finds its own row's entries"""
    from sin_inn_amd import flowcaps, flownet
    for name, row in flowcaps.TABLE.items():
        net = flownet.flow_model_dict[name](flownet.ModelParams())
        enc = getattr(net, 'encode', None)
        assert (getattr(enc, 'kind', None), net.is_progressive, net.encoding_dim) == (row.kind, row.progressive, row.width), name
        assert row.learnable == isinstance(enc, flownet.RotatedFourierFeatures) == any(p is getattr(enc, 'frequencies', None)
                                                                                         for p in net.parameters()), name
        found = flownet._row(net)[1]
        assert (found.pair, found.jacobian) == (row.pair, row.jacobian), name
        assert row.pose_grad is flowcaps.OK and (row.enc_grad is flowcaps.OK) == (row.kind == flowcaps.FOURIER), name
        assert row.spatial is flowcaps.OK or not row.progressive or name == 'PPE', name


def test_refuse_is_silent_or_the_prefixed_reason():
    from sin_inn_amd import flowcaps
    assert flowcaps.refuse(flowcaps.TABLE['PRBF'], 'jacobian', 'anything') is None
    with pytest.raises(ValueError) as e:
        flowcaps.refuse(flowcaps.TABLE['PPE'], 'pair', 'domain_dim 2')
    assert str(e.value) == 'domain_dim 2: ' + flowcaps.P_PE


def test_parsing_needs_no_torch():
    code = ('import importlib.util, os, sys\n'
            'for name, parts in (("flowcaps", ("sin-inn_amd", "flowcaps.py")), ("flow_main", ("video-interpolation", "main.py"))):\n'
            '    spec = importlib.util.spec_from_file_location(name, os.path.join(sys.argv[1], *parts))\n'
            '    mod = importlib.util.module_from_spec(spec)\n'
            '    spec.loader.exec_module(mod)\n'
            'args = mod.get_args(["train", "--net", "PFF", "--spatially-adaptive"])\n'
            'assert args.net == "PFF" and "torch" not in sys.modules, sorted(sys.modules)\n')
    subprocess.run([sys.executable, '-c', code, ROOT], check=True, timeout=60)
