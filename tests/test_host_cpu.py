"""CPU: the C ABI loads and exports every declared symbol, host-side logic (graph lowering, sampler index
arithmetic, TCR matrices, CLI), and the data-parallel glue with world_size 2 on gloo."""
import os
import re
import subprocess
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_every_declared_symbol():
    import sin_inn_amd
    from sin_inn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'sininn.h')).read()
    declared = set(re.findall(r'\b(sininn_[a-z0-9_]+)\s*\(', header))
    declared -= {'sininn_conv_args'}
    handle = _lib.lib()
    for name in sorted(declared):
        assert hasattr(handle, name), f'{name} declared in include/sininn.h but not exported'
    assert declared <= set(_lib.EXPORTED) | {'sininn_conv_args'}
    assert handle.sininn_version() == 4


def _header_prototypes():
    """{name: (return type, [parameter declarations])} of every sininn_* function include/sininn.h declares."""
    text = open(os.path.join(ROOT, 'include', 'sininn.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = re.sub(r'^[ \t]*#[^\n]*(\\\n[^\n]*)*', ' ', text, flags=re.M)        # #define / #include / #ifdef lines
    text = re.sub(r'(\btypedef\s+)?\b(struct|enum)\b[^;{}()]*\{[^{}]*\}[^;]*;', ' ', text)   # struct typedefs and enums
    protos = {}
    for ret, name, params in re.findall(r'([A-Za-z_][\w \t\n\*]*?)\b(sininn_\w+)\s*\(([^()]*)\)\s*;', text):
        assert name not in protos, f'{name} is declared twice'
        params = [p.strip() for p in params.split(',')]
        protos[name] = (' '.join(ret.split()), [] if params == ['void'] else params)
    return protos


def _c_class(decl, is_return=False):
    if '*' in decl or '[' in decl:
        return 'pointer'
    words = [w for w in decl.split() if w != 'const']
    if not is_return:
        words = words[:-1]                                   # the parameter's name
    base = ' '.join(words)
    return {'int': 'int', 'unsigned': 'int', 'unsigned int': 'int', 'int64_t': 'int64', 'size_t': 'size_t', 'float': 'float',
            'double': 'double', 'void': 'void'}[base]


def _ctypes_class(t):
    import ctypes as C
    from sin_inn_amd import _lib
    if t is None:
        return 'void'
    if t in (C.c_void_p, C.c_char_p, _lib.I64x4) or issubclass(t, (C._Pointer, C.Array)):
        return 'pointer'
    return {C.c_int: 'int', C.c_uint: 'int', C.c_int64: 'int64', C.c_size_t: 'size_t', C.c_float: 'float', C.c_double: 'double'}[t]


def test_sigs_agree_with_the_header():
    # needs no built library: the prototypes of include/sininn.h against the ctypes signatures of _lib._SIGS, class by class
    import sin_inn_amd
    from sin_inn_amd import _lib
    protos = _header_prototypes()
    assert len(protos) > 100 and 'sininn_flow_error_stash' in protos and 'sininn_version' in protos
    missing = sorted(set(_lib._SIGS) - set(protos))
    assert not missing, f'_SIGS names that include/sininn.h does not declare: {missing}'
    rowless = sorted(set(protos) - set(_lib._SIGS))
    assert not rowless, f'prototypes of include/sininn.h without a row in _SIGS: {rowless}'
    # the undeclared test hooks are the other table; one that the header comes to declare belongs in _SIGS, where it is checked
    declared_hooks = sorted(set(_lib._TEST_HOOKS) & set(protos))
    assert not declared_hooks, f'_TEST_HOOKS names that include/sininn.h declares (move them to _SIGS): {declared_hooks}'
    assert not set(_lib._TEST_HOOKS) & set(_lib._SIGS) and set(_lib.EXPORTED) == set(_lib._SIGS) | set(_lib._TEST_HOOKS)
    wrong = []
    for name in sorted(set(protos) & set(_lib._SIGS)):
        ret, params = protos[name]
        res, args = _lib._SIGS[name]
        want = [_c_class(ret, True)] + [_c_class(p) for p in params]
        got = [_ctypes_class(res)] + [_ctypes_class(t) for t in args]
        if want != got:
            where = next((i for i, (a, b) in enumerate(zip(want, got)) if a != b), min(len(want), len(got)))
            wrong.append(f'{name}: header {len(params)} parameters, _SIGS {len(args)}; first difference at position {where - 1} '
                         f'(-1 = return): header {want[where:where + 1]}, _SIGS {got[where:where + 1]}')
    assert not wrong, '\n'.join(wrong)


def test_cpu_tensors_are_refused_loudly():
    import sin_inn_amd
    from sin_inn_amd import ops
    with pytest.raises(NotImplementedError):
        ops.ptr(torch.zeros(4))
    import loss
    with pytest.raises(NotImplementedError):
        loss.reconstruction(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2))


def test_coupling_colmap_layout():
    import ctypes as C
    import sin_inn_amd
    from sin_inn_amd import _lib
    buf = (C.c_int * 48)()
    _lib.lib().sininn_coupling_colmap(24, 16, buf)
    m = list(buf)
    assert m[:8] == list(range(8)) and m[8:16] == list(range(24, 32)) and m[16:24] == list(range(8, 16))
    assert sorted(m) == list(range(48))
    buf = (C.c_int * 192)()
    _lib.lib().sininn_coupling_colmap(96, 32, buf)
    m = list(buf)
    assert m[:16] == list(range(16)) and m[16:32] == list(range(96, 112)) and m[32:48] == list(range(16, 32))
    assert sorted(m) == list(range(192))


def _opt(**kw):
    d = dict(scale=4, num_coupling=3, lr_window=1, architecture='SRF', gpu_ids=[0], rotation=5.0, translation=5.0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_graph_lowering_folds_all_permutes():
    import archs
    net = archs.UncondSRFlow(3, 64, 64, _opt())
    fwd = net._lower(False)
    kinds = [k for k, _ in fwd]
    assert kinds == ['squeeze'] + ['glow'] * 3 + ['squeeze'] + ['glow'] * 3
    assert fwd[0][1]['levels'] == 2 and all(p['perm'] is not None for k, p in fwd if k == 'glow')
    rev = net._lower(True)
    kinds = [k for k, _ in rev]
    # only the very first inverse permute (applied to the network input) stays a standalone gather
    assert kinds == ['permute'] + ['glow'] * 3 + ['squeeze'] + ['glow'] * 3 + ['squeeze']
    assert rev[4][1]['perm'] is not None and rev[4][1]['levels'] == 1 and rev[8][1]['levels'] == 2
    assert [p['perm'] is not None for k, p in rev if k == 'glow'] == [True, True, False, True, True, False]
    keys = list(net.state_dict().keys())
    assert keys[0] == 'module_list.3.s1.0.weight' and len(keys) == 6 * 8


def test_same_seed_same_weights_as_oracle():
    import archs
    from oracle import sininn_oracle as O
    torch.manual_seed(0)
    net = archs.UncondSRFlow(3, 64, 64, _opt(num_coupling=2))
    torch.manual_seed(0)
    ref = O.SRFlowOracle(3, 64, 64, num_coupling=2)
    for (ka, a), (kb, b) in zip(net.state_dict().items(), ref.state_dict().items()):
        assert ka == kb and torch.equal(a, b)


def test_dataset_index_arithmetic_and_cli():
    import main
    from data import ConcatDataset, VideoAllDataset, VideoTrainDataset, VideoValDataset
    from oracle import sininn_oracle as O
    a = main.get_args(['train', '--synthetic', '300', '16', '16', '--fps', '10', '--lr_window', '2'])
    assert (a.lr_dims, a.z_dims) == (20, 172)
    sup, unsup = VideoTrainDataset(a), VideoAllDataset(a)
    n = a.frame_store.num_lr
    assert sup.frames == O.train_indices(n, 10) and unsup.frames == O.all_indices(n, 10)
    torch.manual_seed(3)
    val = VideoValDataset(a, 7)
    torch.manual_seed(3)
    assert val.frames == O.val_indices(n, 10, 2, 7, torch.randperm(n - 4).tolist())
    cd = ConcatDataset(sup, unsup)
    assert len(cd) == len(sup) and all(0 <= p < len(unsup) for p in cd.pair_positions(range(5)))
    b = main.get_args(['train', '--synthetic', '8', '64', '64', '--fps', '1', '--lr_window', '1', '--tcr_iters', '3'])
    assert VideoTrainDataset(b).frames == [2] and isinstance(b.tcr_iters, int)


def test_tcr_matrices_match_oracle():
    import tcr
    from oracle import sininn_oracle as O
    rand = torch.rand(5, 3)
    for scale in (1, 0.25):
        m = tcr.pixel_matrix(rand, 12, 20, 5.0, 5.0, scale)
        assert torch.allclose(m, O.tcr_matrix(rand, 12, 20, 5.0, 5.0, scale), atol=1e-6)
        assert torch.allclose(tcr.normalized_inverse(m, 12, 20), O.tcr_theta(m, 12, 20), atol=1e-6)


_DP_SCRIPT = r'''
import os, sys, torch
sys.path.insert(0, %r)
import sin_inn_amd
from sin_inn_amd import dist as sd
rank, ws = sd.init_from_env('gloo')
assert ws == 2
g = torch.full((10,), float(rank + 1))
sd.allreduce_mean_([g])
assert torch.allclose(g, torch.full((10,), 1.5))
w = torch.full((4,), float(rank))
sd.broadcast_([w])
assert torch.equal(w, torch.zeros(4))
assert sd.shard_indices(list(range(8))) == list(range(8))[rank::2]
import data
st = data.FrameStore.synthetic(40, 16, 16)
class D(torch.utils.data.Dataset):
    store = st; frames = list(range(3, 35)); win_size = 1; shuffle = False
    def __len__(self): return len(self.frames)
    def batch(self, pos): return [self.frames[p] for p in pos]
class L(data.DeviceLoader):
    def _store(self): return types.SimpleNamespace(device=types.SimpleNamespace(type='cuda'))
import types
seen = [x for b in L(D(), 4) for x in b]
assert seen == D.frames[rank::2], seen
# ADVICE r1: a length that does not divide by the world size must still give every rank the same number of batches (and
# the same last-batch size), or one rank issues an extra gradient all-reduce and the job hangs
class D41(D):
    frames = list(range(3, 44))
batches = list(L(D41(), 4))
assert len(batches) == len(L(D41(), 4)) == 6 and [len(b) for b in batches] == [4, 4, 4, 4, 4, 1], batches
mine = [x for b in batches for x in b]
assert mine == (D41.frames + D41.frames[:1])[rank::2]
sys.stdout.write(f'rank {rank} ok\n'); sys.stdout.flush()      # one write: the two ranks share the pipe
'''


def test_data_parallel_glue_world2_gloo(tmp_path):
    from conftest import free_port
    script = tmp_path / 'dp.py'
    script.write_text(_DP_SCRIPT % ROOT)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1')
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                          '--master-addr', '127.0.0.1', '--master-port', str(free_port()), str(script)],
                         capture_output=True, text=True, env=env, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'rank 0 ok' in out.stdout and 'rank 1 ok' in out.stdout


@pytest.mark.parametrize('n', [2, 8])
def test_bench_self_launches_its_ranks_cpu_rehearsal(n):
    """`python bench.py --gpus N` with no WORLD_SIZE must spawn its own ranks (torch.distributed.run children, before any
    GPU call) and relay rank 0's JSON line; --rehearse runs that plumbing on gloo without kernels.  The line describes the job it
    came from: world size, backend, one record per rank, the collective, max-over-ranks step time -- for the
    day an 8-GPU node runs it (reference parallelism: main.py:112 Trainer(gpus=...))."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    for attempt in range(3):        # the launcher picks a free port and hands it to torchrun: further tries cover the rare race for it
        if attempt:                 # (and a box that is busy with something else: 8 ranks import torch on 8 cores)
            import time
            time.sleep(2.0)
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', str(n), '--rehearse', '--steps', '3', '--config', '2'],
                             capture_output=True, text=True, env=env, timeout=600)
        if out.returncode == 0:
            break
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == 1, out.stdout      # stdout is the JSON line alone: what gloo / the launcher print goes to stderr (bench.claim_stdout)
    rec = json.loads(lines[0])
    assert rec['n_gpus'] == n and rec['steps'] == 3 and rec['rehearsal'] is True and rec['scaling'] == 'weak'
    assert rec['config']['global_batch'] == 16 * n and rec['config']['parallelism'] == f'dp{n}'
    d = rec['distributed']
    assert d['world_size'] == n and d['backend'] == 'gloo' and len(d['ranks']) == n
    assert sorted(r['rank'] for r in d['ranks']) == list(range(n)) and len({r['pid'] for r in d['ranks']}) == n
    assert d['ms_per_step_max_over_ranks'] > 0 and 'all-reduce' in d['collective']


def test_bench_dump_outputs_writes_floats_and_a_fixed_sample_of_large_arrays(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float64 stays float64, everything else is written as float32; an array above DUMP_MAX_ELEMS is
    written as the same seeded sample (ascending positions) every time, so that two builds' dumps line up element by element."""
    import numpy as np
    import bench
    monkeypatch.setattr(bench, 'DUMP_MAX_ELEMS', 1000)
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), {'big': torch.arange(5000, dtype=torch.float32), 'small': torch.ones(2, 5, dtype=torch.float16),
                                                 'loss': torch.tensor(2.5, dtype=torch.float64)})
    big = np.load(tmp_path / 'a' / 'big.npy')
    assert big.dtype == np.float32 and big.shape == (1000,) and np.array_equal(big, np.load(tmp_path / 'b' / 'big.npy'))
    assert (np.diff(big) > 0).all() and big[0] >= 0 and big[-1] < 5000
    small, loss = np.load(tmp_path / 'a' / 'small.npy'), np.load(tmp_path / 'a' / 'loss.npy')
    assert small.dtype == np.float32 and small.shape == (10,) and (small == 1).all()
    assert loss.dtype == np.float64 and loss.shape == (1,) and loss[0] == 2.5


def test_checkpoint_holds_tensors_and_primitives_only(tmp_path):
    """a checkpoint must load back (torch.load default weights_only=True) and must not carry the clip."""
    import argparse
    import sin_inn_amd
    from sin_inn_amd import lightning as pl
    import data

    class Tiny(pl.LightningModule):
        def __init__(self, c, opt):
            super().__init__()
            self.save_hyperparameters()
            self.lin = torch.nn.Linear(3, 2)

    opt = argparse.Namespace(scale=4, adam_betas=[0.9, 0.99], scene='x', resume_state=None,
                             frame_store=data.FrameStore.synthetic(4, 16, 16))
    m = Tiny(3, opt)
    tr = pl.Trainer.__new__(pl.Trainer)
    tr.current_epoch, tr.global_step = 3, 17
    tr.optimizer = types.SimpleNamespace(state_dict=lambda: {'flat': [dict(m=torch.zeros(4), v=torch.ones(4), step=5)],
                                                             'param_groups': [{'lr': 1e-4, 'betas': (0.9, 0.99)}]})
    path = str(tmp_path / 'ck' / 'epoch=3.ckpt')
    tr.save_checkpoint(m, path)
    assert os.path.getsize(path) < 20000                       # the uint8 clip is not in there
    ck = torch.load(path)                                      # default weights_only=True must work
    assert set(ck['state_dict']) == {'lin.weight', 'lin.bias'} and ck['epoch'] == 3 and ck['global_step'] == 17
    hp = ck['hyper_parameters']
    assert hp['c'] == 3 and hp['opt']['scale'] == 4 and hp['opt']['adam_betas'] == [0.9, 0.99]
    assert 'frame_store' not in hp['opt']
    assert pl.load_checkpoint(path)['optimizer_states'][0]['flat'][0]['step'] == 5
    # a Lightning checkpoint as the reference writes it: argparse.Namespace pickled under hyper_parameters
    ref_path = str(tmp_path / 'ref.ckpt')
    torch.save({'state_dict': m.state_dict(), 'hyper_parameters': {'opt': argparse.Namespace(scale=4)}, 'epoch': 1}, ref_path)
    assert pl.load_checkpoint(ref_path)['hyper_parameters']['opt'].scale == 4
    # anything beyond tensors / primitives / argparse.Namespace is never imported or run: the entry that holds it is dropped
    # (unless the caller opts in to the full unpickler explicitly)
    other = str(tmp_path / 'other.ckpt')
    torch.save({'state_dict': m.state_dict(), 'hyper_parameters': {'opt': types.SimpleNamespace(scale=4), 'c': 3}}, other)
    ck = pl.load_checkpoint(other)
    assert ck['hyper_parameters'] == {'c': 3} and set(ck['state_dict']) == {'lin.weight', 'lin.bias'}
    assert pl.load_checkpoint(other, trust=True)['hyper_parameters']['opt'].scale == 4


def test_reference_style_lightning_checkpoint_loads_without_lightning(tmp_path):
    """pytorch_lightning 1.2's ModelCheckpoint stores `callbacks: {<class ModelCheckpoint>: state}` -- dict keys that
    are pickled class globals of a package that is not installed here.  The file must still resume (the entry is dropped,
    nothing from the file is imported or executed); a file with no usable state_dict says --trust_checkpoint."""
    import argparse
    import pickle
    from sin_inn_amd import lightning as pl
    mod = types.ModuleType('fake_lightning_callbacks')

    class ModelCheckpoint:
        pass
    ModelCheckpoint.__module__, ModelCheckpoint.__qualname__ = mod.__name__, 'ModelCheckpoint'
    mod.ModelCheckpoint = ModelCheckpoint
    sys.modules[mod.__name__] = mod
    sd = {'inn.w': torch.arange(6.0).reshape(2, 3), 'inn.b': torch.ones(2)}
    path = str(tmp_path / 'epoch=99.ckpt')
    try:
        torch.save({'epoch': 99, 'global_step': 1234, 'pytorch-lightning_version': '1.2.0', 'state_dict': sd,
                    'callbacks': {ModelCheckpoint: {'best_model_score': torch.tensor(0.5), 'best_model_path': 'x.ckpt'}},
                    'optimizer_states': [{'state': {0: {'step': 7, 'exp_avg': torch.zeros(3)}}, 'param_groups': [{'lr': 1e-4}]}],
                    'lr_schedulers': [], 'hyper_parameters': {'c': 3, 'opt': argparse.Namespace(scale=4, fps=10)}}, path)
    finally:
        del sys.modules[mod.__name__]                 # as on a box without pytorch_lightning: the global cannot be imported
    with pytest.raises(Exception):
        torch.load(path, weights_only=False)          # the plain unpickler needs the package
    ck = pl.load_checkpoint(path)
    assert ck['epoch'] == 99 and ck['global_step'] == 1234 and ck['callbacks'] == {}
    assert torch.equal(ck['state_dict']['inn.w'], sd['inn.w']) and ck['hyper_parameters']['opt'].fps == 10
    assert ck['optimizer_states'][0]['state'][0]['step'] == 7
    # code in a file is never run by the default path: a reduce that would call os.system resolves to an inert stand-in
    marker = tmp_path / 'ran'

    class Boom:
        def __reduce__(self):
            return (os.system, (f'touch {marker}',))
    bad = str(tmp_path / 'bad.ckpt')
    torch.save({'state_dict': sd, 'payload': Boom()}, bad)
    ck = pl.load_checkpoint(bad)
    assert not marker.exists() and 'payload' not in ck and set(ck['state_dict']) == set(sd)
    # nothing usable left -> the error names the opt-in
    empty = str(tmp_path / 'empty.ckpt')
    torch.save({'state_dict': Boom()}, empty)
    with pytest.raises(pickle.UnpicklingError, match='--trust_checkpoint'):
        pl.load_checkpoint(empty)
    assert not marker.exists()


def test_test_mode_loads_strictly_and_tolerates_only_freia_bookkeeping():
    import main
    net = torch.nn.Sequential(torch.nn.Linear(2, 2))
    good = {k: v.clone() for k, v in net.state_dict().items()}
    main.load_weights(net, good)
    main.load_weights(net, dict(good, **{'module_list.4.perm': torch.arange(3), 'module_list.4.perm_inv': torch.arange(3)}))
    with pytest.raises(SystemExit):
        main.load_weights(net, {'0.weight': good['0.weight']})                 # a real parameter is missing
    with pytest.raises(SystemExit):
        main.load_weights(net, dict(good, **{'1.weight': torch.zeros(2, 2)}))  # wrong architecture
    main.load_weights(net, {'0.weight': good['0.weight']}, allow_partial=True)


def _write_png_tree(root, scene, t, h, w, skip_lr=(), skip_hr=()):
    from PIL import Image
    import numpy as np
    rng = np.random.RandomState(0)
    hr = rng.randint(0, 256, (t, h, w, 3), dtype=np.uint8)
    lr = rng.randint(0, 256, (t, h // 8, w // 8, 4), dtype=np.uint8)
    for kind in ('hr_frames', 'lr_frames'):
        os.makedirs(os.path.join(root, kind, scene), exist_ok=True)
    for i in range(t):
        if i not in skip_lr:
            Image.fromarray(lr[i], 'RGBA').save(os.path.join(root, 'lr_frames', scene, f'frame_{i:05d}.png'))
        if i not in skip_hr:
            Image.fromarray(hr[i], 'RGB').save(os.path.join(root, 'hr_frames', scene, f'frame_{i:05d}.png'))
    return hr, lr


def test_frame_store_from_directory_layout_and_missing_frames(tmp_path):
    """<dataset>/{hr_frames,lr_frames}/<scene>/frame_%05d.png (data.py:20-21,57-59); a missing PNG fails loudly like the
    reference's io.imread instead of leaving a zero frame."""
    import numpy as np
    import data
    hr, lr = _write_png_tree(str(tmp_path / 'ok'), 'clip', 30, 16, 16)
    st = data.FrameStore.from_directory(str(tmp_path / 'ok'), 'clip')
    assert st.num_lr == 29 and np.array_equal(st.hr.numpy(), hr) and np.array_equal(st.lr.numpy(), lr)
    opt = types.SimpleNamespace(fps=10, lr_window=1, operation='train', dataset=str(tmp_path / 'ok'), scene='clip')
    assert data.VideoTrainDataset(opt).frames == list(range(11, 19, 12))
    assert opt.frame_store is not None                                          # decoded once, shared
    # HR frames exist only where the reference would read them: sparse HR directories are fine ...
    _write_png_tree(str(tmp_path / 'sparse'), 'clip', 30, 16, 16, skip_hr=set(range(30)) - {11})
    opt2 = types.SimpleNamespace(fps=10, lr_window=1, operation='train', dataset=str(tmp_path / 'sparse'), scene='clip')
    assert data.VideoTrainDataset(opt2).frames == [11]
    with pytest.raises(FileNotFoundError):                                       # ... but not for a dataset that needs them
        data.VideoAllDataset(opt2)
    _write_png_tree(str(tmp_path / 'gap'), 'clip', 30, 16, 16, skip_lr={12})
    with pytest.raises(FileNotFoundError):
        data.FrameStore.from_directory(str(tmp_path / 'gap'), 'clip')


def test_descriptor_guards_refuse_before_any_launch():
    """ABI v4 guards against the cause of round 2's abort: a descriptor that was not zeroed + size-tagged, a channel
    gap outside the operand, or a DenseBlock buffer smaller than the launch sequence needs is refused with an error message
    BEFORE anything is launched (so this runs without a GPU; the pointers are never dereferenced)."""
    import ctypes as C
    import sin_inn_amd
    from sin_inn_amd import _lib
    lib = _lib.lib()
    for which, mirror in enumerate((_lib.ConvArgs, _lib.WgradItem, _lib.DenseArgs, _lib.GlowArgs, _lib.SubnetArgs, _lib.PackDesc)):
        assert lib.sininn_sizeof(which) == C.sizeof(mirror)
    fake = 0x7f0000000000                         # 16-byte aligned, never dereferenced on the host
    arr = (_lib.WgradItem * 2)()
    for it in arr:
        it.inp, it.dout, it.gw = fake, fake, fake
        it.in_stride, it.Cin, it.dout_stride, it.N = 64, 64, 32, 32
    # 1. untagged items (what a caller built against the v3 header, or a field-by-field fill of a grown struct, hands over)
    assert lib.sininn_wgrad_group_workspace_bytes(arr, 2, 1, 16, 16, 3) == 0
    assert b'struct_bytes' in lib.sininn_last_error()
    assert lib.sininn_wgrad_group(arr, 2, 1, 16, 16, 3, fake, 1 << 30, None) != 0
    for it in arr:
        it.struct_bytes = C.sizeof(_lib.WgradItem)
    assert lib.sininn_wgrad_group_workspace_bytes(arr, 2, 1, 16, 16, 3) > 0
    # 2. garbage in the optional fields (the uninitialised gap_begin / gap_len of the abort)
    arr[1].gap_begin, arr[1].gap_len = 60, 0x40000000
    assert lib.sininn_wgrad_group(arr, 2, 1, 16, 16, 3, fake, 1 << 30, None) != 0
    assert b'channel gap' in lib.sininn_last_error()
    arr[1].gap_begin, arr[1].gap_len = -8, 8
    assert lib.sininn_wgrad_group(arr, 2, 1, 16, 16, 3, fake, 1 << 30, None) != 0
    arr[1].gap_begin, arr[1].gap_len = 0, 0
    arr[0].in_bf16 = 7
    assert lib.sininn_wgrad_group(arr, 2, 1, 16, 16, 3, fake, 1 << 30, None) != 0
    assert b'dtype flags' in lib.sininn_last_error()
    # 3. DenseBlock executor: undersized buffers
    m, cin, cout = 2 * 8 * 8, 12, 20
    bw = 16 + 128

    def dense(**over):
        a = _lib.DenseArgs(B=2, H=8, W=8, cin=cin, cout=cout, mode=2, winograd=1, clamp=1.0)
        a.x, a.x_stride, a.aux1, a.aux1_stride, a.aux2, a.buf, a.out = fake, cin, fake, cout, fake, fake, fake
        for i in range(5):
            a.w_fwd[i] = a.b_fwd[i] = a.w_dgrad[i] = fake
        a.buf_floats, a.out_floats, a.aux2_floats = m * bw, m * cout, m * cout
        a.dout, a.dF, a.dD, a.dh, a.dv, a.workspace = fake, fake, fake, fake, fake, fake
        a.dout_floats, a.dF_floats, a.dD_floats, a.dh_floats, a.dv_floats = m * cout, m * bw, m * 24, m * cout, m * cout
        a.workspace_bytes = 1 << 30
        for k, v in over.items():
            setattr(a, k, v)
        return a
    for fn, over, word in ((lib.sininn_dense_forward, dict(buf_floats=m * bw - 1), b'buf holds'),
                           (lib.sininn_dense_forward, dict(out_floats=m * cout - 4), b'out holds'),
                           (lib.sininn_dense_forward, dict(aux2_floats=0), b'aux2 holds'),
                           (lib.sininn_dense_forward, dict(struct_bytes=C.sizeof(_lib.DenseArgs) - 64), b'struct_bytes'),
                           (lib.sininn_dense_backward, dict(dF_floats=m * (bw - 8)), b'dF holds'),
                           (lib.sininn_dense_backward, dict(dD_floats=m * cout), b'dD holds'),     # needs pad8(cout) = 24 columns
                           (lib.sininn_dense_backward, dict(dh_floats=m), b'dh / dv hold'),
                           (lib.sininn_dense_backward, dict(dout_floats=m), b'dout holds')):
        a = dense(**over)
        rc = fn(a, None) if fn is lib.sininn_dense_forward else fn(a, None, None)
        assert rc != 0 and word in lib.sininn_last_error(), (over, lib.sininn_last_error())


def test_mmd_gram_refuses_batches_beyond_its_lds_staging():
    """mmd_gram stages 2 * B * 129 floats of LDS per block: batches outside 1..64 are refused with the ordinary error return before
    anything is launched (B == 64 itself, 66 048 bytes, is checked against the device's per-block limit at launch time:
    tests/test_gpu_elementwise_sizes.py)."""
    import sin_inn_amd
    from sin_inn_amd import _lib
    lib = _lib.lib()
    fake = 0x7f0000000000                         # never dereferenced on the host
    st = _lib.I64x4(48, 16, 4, 1)
    for b in (65, 128, 0, -1):
        assert lib.sininn_mmd_gram(fake, st, fake, st, b, 3, 4, 4, fake, None) != 0
        assert b'batch must be in 1..64' in lib.sininn_last_error()
    assert lib.sininn_mmd_finish(fake, 65, 0, fake, fake, None) != 0


def test_32_bit_staging_offsets_are_range_checked_on_the_host():
    """Round 3 moved the staging loops to 32-bit byte offsets (raw buffer loads inside one image, per-tile descriptors in the
    weight gradient): shapes those offsets cannot address are refused before any launch (no GPU needed)."""
    import ctypes as C
    import sin_inn_amd
    from sin_inn_amd import _lib
    lib = _lib.lib()
    fake = 0x7f0000000000
    # weight gradient: a pixel tile whose rows are 2^24 pixels x 256 floats apart
    rc = lib.sininn_wgrad(fake, 256, 256, fake, 256, 256, 1, 8, 1 << 24, 3, fake, None, fake, 1 << 40, None)
    assert rc != 0 and b'32-bit staging offsets' in lib.sininn_last_error(), lib.sininn_last_error()
    # Winograd conv: one image of 2048 x 2048 pixels x 256 floats = 4 GB (its element count still fits the older 2^31 check)
    a = _lib.ConvArgs(B=1, H=2048, W=2048, ksize=3, Cin=256, in_stride=256, Np=32, N=32, out_stride=32, winograd=1, mode=_lib.CONV_LINEAR)
    a.inp, a.w, a.out = fake, fake, fake
    rc = lib.sininn_conv(C.byref(a), None)
    assert rc != 0 and b'exceeds the 2 GB' in lib.sininn_last_error(), lib.sininn_last_error()


def test_group_major_layout_is_chosen_only_where_the_kernels_can_address_it():
    """the executor's layout predicate must imply the kernels' own range checks -- a shape beyond them takes the
    row-major hidden layout instead of failing in sininn_conv with 'channel-group stride too large' (host-only, no launch)."""
    import ctypes as C
    import sin_inn_amd
    from sin_inn_amd import _lib
    lib = _lib.lib()
    fake = 0x7f0000000000
    assert lib.sininn_glow_group_major_fits(16, 64, 64) == 1 and lib.sininn_glow_group_major_fits(16, 180, 320) == 1   # cfg 1 / 4
    assert lib.sininn_glow_group_major_fits(16, 512, 512) == 0 and lib.sininn_glow_group_major_fits(16, 1024, 1024) == 0

    def conv_refuses_stride(b, h, w):
        a = _lib.ConvArgs(B=b, H=h, W=w, ksize=3, Cin=256, in_stride=8, Np=64, N=64, out_stride=64, winograd=1, mode=_lib.CONV_LINEAR)
        a.in_group_stride = b * h * w * 8 if b * h * w * 8 < 2 ** 31 else 2 ** 31 - 8
        a.inp, a.w, a.out = fake, fake, fake
        rc = lib.sininn_conv(C.byref(a), None)
        return rc != 0 and b'group stride too large' in lib.sininn_last_error()
    for b, h, w in ((16, 64, 64), (16, 256, 256), (15, 512, 512), (16, 511, 512), (16, 512, 512), (3, 1200, 1160), (1, 2040, 2040)):
        fits = lib.sininn_glow_group_major_fits(b, h, w) == 1
        assert not (fits and conv_refuses_stride(b, h, w)), (b, h, w)       # chosen => addressable
    assert conv_refuses_stride(16, 512, 512)                                # the check the predicate has to stay inside


def test_frame_store_refuses_a_clip_that_does_not_start_at_frame_0(tmp_path):
    """the reference indexes frame_{x:05d}.png from 0 (data.py:33-38): LR frames missing BEFORE the first present index are a
    gap too (they would otherwise sit in neighbouring frames' LR windows as all-zero planes)"""
    import data
    _write_png_tree(str(tmp_path / 'late'), 'clip', 30, 16, 16, skip_lr={0, 1})
    with pytest.raises(FileNotFoundError, match='frame_00000.png'):
        data.FrameStore.from_directory(str(tmp_path / 'late'), 'clip')
