"""GPU: the IRN architecture in mixed precision (`-a IRN --precision bf16`).  Contract (irn.InvRescaleNet.set_precision):
the DenseBlock convs compute in bf16 with fp32 accumulation, the feature buffer [pixels][pad8(cin) + 128] and the weight packs
are bf16, conv5's output, the InvBlockExp tails, Haar, the losses and every gradient stay fp32; the gradients that feed a
data-gradient or weight-gradient conv (dD, each finished dF slot) are rounded to bf16 while staged.

The bf16 emulation here (float64 arithmetic) rounds exactly at the contract's points: the block input, conv1-4's outputs
after LeakyReLU, the five weights (bf16_round, straight-through gradients), and the gradient of every conv's output
(_RoundGrad: identity forward, bf16-rounded gradient).

Tolerances (stated up front, in the style of tests/test_gpu_bf16.py):
  * kernels whose operands are bf16 on both sides differ from float64 only by fp32 accumulation order: 1e-4 of the max-norm
    for fp32 outputs; one bf16 ulp (2^-7 relative) for the bf16 feature slot;
  * a DenseBlock / InvBlockExp against the emulation, LeakyReLU gates forced from the HIP pass (GATE_TAP): outputs 2e-2
    max-norm / 3e-3 L2 (a feature value on a bf16 rounding boundary lands on the other side and is carried on), input
    gradients 5e-2 max-norm / 2e-2 L2, per-tensor parameter gradients 5e-2 L2 (the weight gradients also sum bf16-rounded
    products in another order);
  * the whole InvRescaleNet: every block against the emulation on its own HIP input, 2e-2 max-norm / 3e-3 L2; the inverse
    of the forward returns x to 5e-3 L2 (the two directions round different features); against the fp32 HIP path, for the
    record: 5e-2 L2."""
import ctypes as C
import glob
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return bf(g)


def emu_dense(convs, x, gates=None):
    """bf16 emulation of one DenseBlock (archs.py:74-98) in float64; convs = the five (weight, bias) leaf tensors."""
    from oracle.sininn_oracle import bf16_round
    feats = [bf16_round(x)]
    for i, (w, b) in enumerate(convs):
        y = _RoundGrad.apply(F.conv2d(torch.cat(feats, 1), bf16_round(w), b, padding=1))
        if i < 4:
            y = y * (0.2 + 0.8 * gates[i].to(y.dtype)) if gates is not None else F.leaky_relu(y, 0.2)
            feats.append(bf16_round(y))
    return y


def leaves(blk):
    """float64 CPU leaf copies of a HIP DenseBlock's parameters, in (weight, bias) pairs"""
    return [(cv.weight.detach().double().cpu().requires_grad_(True), cv.bias.detach().double().cpu().requires_grad_(True))
            for cv in blk.convs()]


def emu_invblock(p, x, l1, clamp, rev, gates):
    x1, x2 = x[:, :l1], x[:, l1:]
    if not rev:
        y1 = x1 + emu_dense(p['F'], x2, gates['F'])
        s = clamp * (torch.sigmoid(emu_dense(p['H'], y1, gates['H'])) * 2 - 1)
        y2 = x2 * torch.exp(s) + emu_dense(p['G'], y1, gates['G'])
    else:
        s = clamp * (torch.sigmoid(emu_dense(p['H'], x1, gates['H'])) * 2 - 1)
        y2 = (x2 - emu_dense(p['G'], x1, gates['G'])) / torch.exp(s)
        y1 = x1 - emu_dense(p['F'], y2, gates['F'])
    return torch.cat((y1, y2), 1)


def _randomise(blk, seed):
    """conv5 is zero-initialised (archs.py:100-132): give every conv non-trivial weights so that each kernel matters"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for cv in blk.convs():
            fan = cv.weight[0].numel()
            cv.weight.copy_(torch.randn(cv.weight.shape, generator=g) * (1.5 / fan) ** 0.5)
            cv.bias.copy_(torch.randn(cv.bias.shape, generator=g) * 0.05)


def _tap(fn):
    """run fn() with GATE_TAP on; return (result, {block: {rev: [four (B,32,H,W) bool gates]}})"""
    from sin_inn_amd.modules import GATE_TAP
    GATE_TAP[0] = []
    try:
        out = fn()
        taps = list(GATE_TAP[0])
    finally:
        GATE_TAP[0] = None
    gates = {}
    for blk, rev, gs in taps:
        gates.setdefault(id(blk), {})[rev] = [g.detach().cpu() for g in gs]
    return out, gates


# ---------------------------------------------------------------------------------------------------------------------
# kernel level: sininn_conv with bf16 packs, against float64 on the same bf16-rounded operands
# ---------------------------------------------------------------------------------------------------------------------
def _vp(t):
    return C.c_void_p(t.data_ptr())


def _pack(w, b):
    from sin_inn_amd import ops
    return ops.pack_conv_bf16(w.contiguous().cuda(), b.contiguous().cuda(), None, True)


def _ref_conv(x_nhwc, w, b=None):
    """float64 conv on NHWC input, NHWC output"""
    y = F.conv2d(x_nhwc.double().cpu().permute(0, 3, 1, 2), w.double().cpu(), None if b is None else b.double().cpu(), padding=1)
    return y.permute(0, 2, 3, 1)


SHAPES = [(1, 16, 16, 24), (2, 13, 21, 88 + 32), (3, 9, 35, 112 + 96), (2, 17, 18, 16), (1, 20, 7, 184 + 64)]


@pytest.mark.parametrize('B,H,W,K', SHAPES)
def test_kernel_lrelu_into_bf16_slot(B, H, W, K):
    """conv1-4: bf16 feature buffer (K channels of a wider row) -> LeakyReLU epilogue -> bf16 slot of the same row."""
    from sin_inn_amd import ops
    g = torch.Generator().manual_seed(K)
    stride = K + 32 + 8
    buf = (torch.randn(B, H, W, stride, generator=g) * 0.5).to(torch.bfloat16).cuda()
    w = torch.randn(32, K, 3, 3, generator=g) * (2.0 / (9 * K)) ** 0.5
    b = torch.randn(32, generator=g) * 0.1
    wf, bfw, _ = _pack(w, b)
    before = buf.clone()
    ops.conv(in_=_vp(buf), in_stride=stride, Cin=K, w=_vp(wf), bias=_vp(bfw), Np=32, B=B, H=H, W=W, ksize=3, mode=6, clamp=0.2,
             out=C.c_void_p(buf.data_ptr() + 2 * K), out_stride=stride, N=32, w_bf16=1, in_bf16=1, out_bf16=1)
    torch.cuda.synchronize()
    want = F.leaky_relu(_ref_conv(before[..., :K].float(), bf(w.double()), b), 0.2)
    got = buf[..., K:K + 32].double().cpu()
    err = (got - want).abs()
    assert bool((err <= 2.0 ** -7 * want.abs() + 1e-6 * want.abs().max()).all()), float(err.max())
    assert torch.equal(buf[..., :K].cpu(), before[..., :K].cpu()) and torch.equal(buf[..., K + 32:].cpu(), before[..., K + 32:].cpu())


@pytest.mark.parametrize('mode', ['linear', 'add', 'irn_fwd', 'irn_inv'])
@pytest.mark.parametrize('B,H,W,cin,cout', [(2, 13, 21, 24, 24), (1, 9, 35, 108, 84), (3, 17, 18, 84, 108), (2, 20, 7, 12, 180)])
def test_kernel_conv5_fp32_tails(mode, B, H, W, cin, cout):
    """conv5: bf16 feature buffer (K = pad8(cin) + 128) -> fp32 out through LINEAR / ADD / IRN_FWD / IRN_INV."""
    from sin_inn_amd import ops
    g = torch.Generator().manual_seed(cin * 7 + cout)
    K = (cin + 7) // 8 * 8 + 128
    coutp = (cout + 7) // 8 * 8
    buf = (torch.randn(B, H, W, K, generator=g) * 0.5).to(torch.bfloat16).cuda()
    w = torch.randn(cout, K, 3, 3, generator=g) * (2.0 / (9 * K)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    wf, bfw, _ = _pack(torch.cat([w, torch.zeros(coutp - cout, K, 3, 3)]), torch.cat([b, torch.zeros(coutp - cout)]))
    aux = torch.randn(B, H, W, cout + 8, generator=g).cuda()             # v / addend: a channel slice of a wider tensor
    hval = torch.randn(B, H, W, cout, generator=g).cuda()
    out = torch.full((B, H, W, cout), float('nan'), device='cuda')
    kw = dict(in_=_vp(buf), in_stride=K, Cin=K, w=_vp(wf), bias=_vp(bfw), Np=(coutp + 15) // 16 * 16, B=B, H=H, W=W, ksize=3,
              out=_vp(out), out_stride=cout, N=cout, w_bf16=1, in_bf16=1)
    vslice = C.c_void_p(aux.data_ptr() + 8 * 4)
    if mode == 'linear':
        kw.update(mode=5)
    elif mode == 'add':
        kw.update(mode=4, addend=vslice, addend_stride=cout + 8)
    else:
        kw.update(mode=7 if mode == 'irn_fwd' else 8, v=vslice, v_stride=cout + 8, mask=_vp(hval), mask_stride=cout, clamp=1.0)
    ops.conv(**kw)
    torch.cuda.synchronize()
    a = _ref_conv(buf.float(), bf(w.double()), b)
    v, hv = aux[..., 8:].double().cpu(), hval.double().cpu()
    s = 1.0 * (2 * torch.sigmoid(hv) - 1)
    want = {'linear': a, 'add': a + v, 'irn_fwd': v * torch.exp(s) + a, 'irn_inv': (v - a) / torch.exp(s)}[mode]
    assert relerr(out, want) < 1e-4


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('B,H,W,Kin,N', [(2, 13, 21, 24, 152), (1, 9, 35, 32, 88 + 96), (3, 17, 18, 112, 240), (2, 20, 7, 32, 48)])
def test_kernel_dgrad_fp32_in_out_bf16_gate(accumulate, B, H, W, Kin, N):
    """data gradients: fp32 input (rounded while staged) -> fp32 output (LINEAR or ADD into itself), LeakyReLU backward on the
    last 32 columns with the gate read from a bf16 feature buffer."""
    from sin_inn_amd import ops
    g = torch.Generator().manual_seed(Kin * 3 + N)
    co = N - 32
    src = torch.randn(B, H, W, Kin + 4, generator=g).cuda()          # a slice of a wider row
    w = torch.randn(Kin, N, 3, 3, generator=g) * (2.0 / (9 * Kin)) ** 0.5      # the conv's OIHW weight: N inputs, Kin outputs
    _, _, wd = _pack(w, torch.zeros(Kin))
    feat = torch.randn(B, H, W, N + 8, generator=g).to(torch.bfloat16).cuda()
    dst0 = torch.randn(B, H, W, N + 8, generator=g).cuda()
    dst = dst0.clone()
    kw = dict(in_=_vp(src), in_stride=Kin + 4, Cin=Kin, w=_vp(wd), Np=(N + 15) // 16 * 16, B=B, H=H, W=W, ksize=3,
              out=_vp(dst), out_stride=N + 8, N=N, w_bf16=1, in_bf16=0, out_bf16=0,
              mask=_vp(feat), mask_bf16=1, mask_stride=N + 8, Co=co, clamp=0.2)
    kw.update(mode=4, addend=_vp(dst), addend_stride=N + 8) if accumulate else kw.update(mode=5)
    ops.conv(**kw)
    torch.cuda.synchronize()
    # the data gradient of a conv with weight w (N in -> Kin out) is the conv of the output gradient with the flipped,
    # transposed weight: conv_transpose2d == conv2d(flip(w).transpose)
    wt = bf(w.double()).flip(2, 3).transpose(0, 1)
    want = _ref_conv(bf(src[..., :Kin].double()), wt)
    if accumulate:
        want = want + dst0[..., :N].double().cpu()
    gate = feat[..., co:N].double().cpu() > 0
    want[..., co:] = torch.where(gate, want[..., co:], want[..., co:] * 0.2)
    assert relerr(dst[..., :N], want) < 1e-4
    assert torch.equal(dst[..., N:].cpu(), dst0[..., N:].cpu())


# ---------------------------------------------------------------------------------------------------------------------
# DenseBlock / InvBlockExp against the emulation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ch,split,B,H,W', [(48, 24, 2, 13, 21), (192, 84, 1, 9, 35), (192, 12, 3, 8, 17)])
@pytest.mark.parametrize('rev', [False, True])
def test_invblockexp_bf16_against_emulation(ch, split, B, H, W, rev):
    """both directions of an InvBlockExp (every tail mode of the executor: ADD, IRN_FWD / IRN_INV, LINEAR) with the gates
    forced from the HIP pass: outputs, dx and all parameter gradients of F, G and H."""
    import archs
    torch.manual_seed(3)
    blk = archs.InvBlockExp(ch, split)
    for i, d in enumerate((blk.F, blk.G, blk.H)):
        _randomise(d, 10 * ch + i)
    blk.cuda()
    for d in (blk.F, blk.G, blk.H):
        d.precision = 'bf16'
    x = torch.randn(B, ch, H, W, generator=torch.Generator().manual_seed(1)) * 0.5
    wgt = torch.randn(B, ch, H, W, generator=torch.Generator().manual_seed(2))
    xg = x.cuda().requires_grad_(True)

    def run():
        y = blk(xg, rev=rev)
        (y * wgt.cuda()).sum().backward()
        return y
    y, gates = _tap(run)
    p = {n: leaves(getattr(blk, n)) for n in 'FGH'}
    gsel = {n: gates[id(getattr(blk, n))][rev] for n in 'FGH'}
    xe = x.double().requires_grad_(True)
    ye = emu_invblock(p, xe, split, blk.clamp, rev, gsel)
    (ye * wgt.double()).sum().backward()
    assert relerr(y, ye) < 2e-2 and rel_l2(y, ye) < 3e-3
    assert relerr(xg.grad, xe.grad) < 5e-2 and rel_l2(xg.grad, xe.grad) < 2e-2
    for n in 'FGH':
        for i, (cv, (we, be)) in enumerate(zip(getattr(blk, n).convs(), p[n])):
            assert rel_l2(cv.weight.grad, we.grad) < 5e-2, (n, i, rel_l2(cv.weight.grad, we.grad))
            assert rel_l2(cv.bias.grad, be.grad) < 5e-2, (n, i, 'bias')


def test_dense_block_bf16_saves_half_the_bytes():
    """the feature buffer a bf16 forward saves for backward is torch.bfloat16 and half the bytes of the fp32 one"""
    import archs
    blk = archs.InvBlockExp(192, 84).cuda()
    x = torch.randn(2, 40, 40, 108, device='cuda', requires_grad=True)
    saved = {}
    for prec in ('fp32', 'bf16'):
        blk.F.precision = prec
        out = blk.F.run(x)
        buf = out.grad_fn.saved_tensors[0]
        assert buf.shape == (2 * 40 * 40, 112 + 128)
        saved[prec] = buf
    assert saved['fp32'].dtype == torch.float32 and saved['bf16'].dtype == torch.bfloat16
    assert saved['bf16'].numel() * saved['bf16'].element_size() * 2 == saved['fp32'].numel() * saved['fp32'].element_size()


# ---------------------------------------------------------------------------------------------------------------------
# whole network, training, CLI
# ---------------------------------------------------------------------------------------------------------------------
def _opt(**kw):
    from test_gpu_model import make_opt
    return make_opt(architecture='IRN', **kw)


@pytest.mark.parametrize('size,num_coupling,lr_window', [(64, 2, 1), (256, 4, 10)])
def test_invrescalenet_bf16_against_emulation_and_roundtrip(size, num_coupling, lr_window):
    """The whole bf16 network, batch 2 (64x64 -c 2; 256x256 -c 4 with lr_window 10, whose level-1 blocks split 84 | 108):
    every InvBlockExp of the HIP forward pass against the bf16 emulation of that block applied to the block's own HIP
    input, gates forced from the HIP pass; the inverse of the forward; the distance to the fp32 HIP path for the record.
    The inverse pass is checked the same way, block by block.  Each block is compared on its HIP input because bf16 rounding boundaries make two evaluations diverge with depth: fed
    its own (emulated) predecessors, the emulation drifts to 4.8e-3 L2 by the fourth block at 64x64 -c 2 while every
    block, compared on its input, stays within 1e-3 L2."""
    import lit_wrapper
    from sin_inn_amd.modules import import_nchw
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    torch.manual_seed(4)
    opt = _opt(num_coupling=num_coupling, lr_window=lr_window, precision='bf16')
    model = lit_wrapper.SingleVideoINN(3, size, size, opt).cuda()
    net = model.inn
    for j, blk in enumerate(net.dense_blocks()):
        _randomise(blk, 100 + j)
    x = torch.rand(2, 3, size, size, generator=torch.Generator().manual_seed(6))

    def forward():                                       # differentiable pass (the gates are recorded), block by block
        seen, out = [], x.cuda()
        for op in net.operations:
            if op.__class__.__name__ == 'HaarDownsampling':
                out = op(out, False)
            else:
                inp = out.detach()
                out = op.apply_pixel_major(import_nchw(out), False).permute(0, 3, 1, 2)
                seen.append((op, inp, out.detach()))
        return out.detach(), seen
    (y, seen), gates = _tap(forward)
    assert len(seen) == 2 * num_coupling
    for op, inp, hip in seen:
        p = {n: [(w.detach(), b.detach()) for w, b in leaves(getattr(op, n))] for n in 'FGH'}
        with torch.no_grad():
            emu = emu_invblock(p, inp.double().cpu(), op.split_len1, op.clamp, False,
                               {n: gates[id(getattr(op, n))][False] for n in 'FGH'})
        assert relerr(hip, emu) < 2e-2 and rel_l2(hip, emu) < 3e-3, (inp.shape, relerr(hip, emu), rel_l2(hip, emu))
    with torch.no_grad():
        assert rel_l2(net(x.cuda()), y) < 1e-6                        # the whole-network call (H beside G, tail kernel)
        # the inverse direction of the no-grad path (H beside G, stand-alone tail), block by block on the blocks' forward
        # outputs (LeakyReLU decided by each side itself: a kink flip moves a value that is itself near 0)
        for op, inp, hip in seen:
            p = {n: [(w.detach(), b.detach()) for w, b in leaves(getattr(op, n))] for n in 'FGH'}
            inv = op.apply_pixel_major(import_nchw(hip), True).permute(0, 3, 1, 2)
            emu = emu_invblock(p, hip.double().cpu(), op.split_len1, op.clamp, True, dict.fromkeys('FGH'))
            assert relerr(inv, emu) < 2e-2 and rel_l2(inv, emu) < 3e-3, (inp.shape, relerr(inv, emu), rel_l2(inv, emu))
        net.set_precision('fp32')
        y32 = net(x.cuda())
    assert rel_l2(y, y32) < 5e-2
    # round trip of the whole network.  With the strong random weights above an 8-block inverse amplifies any rounding
    # (the fp32 flow is exact only for exact subnets); at the reference's initial scale with conv5 live it returns x
    net.set_precision('bf16')
    torch.manual_seed(4)
    fresh = lit_wrapper.SingleVideoINN(3, size, size, opt).cuda().inn
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for blk in fresh.dense_blocks():
            c5 = blk.convs()[4]
            c5.weight.copy_(torch.randn(c5.weight.shape, generator=g) * 0.1 / c5.weight[0].numel() ** 0.5)
        back = fresh(fresh(x.cuda()), rev=True)
    assert rel_l2(back, x) < 5e-3


def test_bf16_training_step_tracks_fp32():
    """one IRN training step in both precisions from the same weights / frames / latents"""
    import lit_wrapper
    from data import FrameStore
    from sin_inn_amd.functional import sample_windows
    results = {}
    for prec in ('fp32', 'bf16'):
        torch.manual_seed(11)
        opt = _opt(num_coupling=2, lr_window=2, precision=prec)
        model = lit_wrapper.SingleVideoINN(3, 64, 64, opt).cuda()
        optim = model.attach_optimizer()
        store = FrameStore.synthetic(12, 64, 64).to('cuda')
        idx = torch.tensor([3, 4, 6, 8]).cuda()
        hr, lr = sample_windows(store.hr, store.lr, idx, 2)
        z = torch.randn(4, opt.z_dims, 8, 8, generator=torch.Generator().manual_seed(2))
        real = lit_wrapper._latent
        lit_wrapper._latent = lambda b, zd, h, w, device, temp=1.0: z.to(device)
        try:
            model.training_step([{'hr': hr, 'lr': lr}, {'hr': hr, 'lr': lr}], 0)
        finally:
            lit_wrapper._latent = real
        results[prec] = (float(model._logged['train']), optim.flat_grads()[0].clone())
    (l32, g32), (l16, g16) = results['fp32'], results['bf16']
    assert abs(l16 / l32 - 1) < 2e-2
    assert rel_l2(g16, g32) < 6e-2
    assert float((g16 * g32).sum() / (g16.norm() * g32.norm())) > 0.998


def test_bf16_short_training_run_loss_falls():
    """40 steps of the bf16 IRN path on a synthetic clip: finite losses, falling"""
    import lit_wrapper
    from data import FrameStore
    from sin_inn_amd.functional import sample_windows
    torch.manual_seed(2)
    opt = _opt(num_coupling=2, lr_window=1, precision='bf16', learning_rate=2e-4)
    model = lit_wrapper.SingleVideoINN(3, 64, 64, opt).cuda()
    model.attach_optimizer()
    store = FrameStore.synthetic(12, 64, 64).to('cuda')
    g = torch.Generator().manual_seed(3)
    losses = []
    for _ in range(40):
        idx = torch.randint(1, 11, (4,), generator=g).cuda()
        hr, lr = sample_windows(store.hr, store.lr, idx, 1)
        model.training_step([{'hr': hr, 'lr': lr}, {'hr': hr, 'lr': lr}], 0)
        losses.append(float(model._logged['train']))
    assert all(torch.isfinite(torch.tensor(losses)))
    first, last = sum(losses[:5]) / 5, sum(losses[-5:]) / 5
    assert last < 0.8 * first, (first, last)


def test_graph_replay_equals_eager_bitwise_irn_bf16():
    """test_gpu_model.test_graph_replay_equals_eager_bitwise for ('IRN', 'bf16')"""
    import test_gpu_model
    test_gpu_model.test_graph_replay_equals_eager_bitwise('IRN', 'bf16')


def test_cli_train_checkpoint_test_irn_bf16(tmp_path):
    """main.py train -a IRN --precision bf16 -> checkpoint -> resume -> test writing frames"""
    import main
    from sin_inn_amd.lightning import load_checkpoint
    wd = str(tmp_path / 'exp')
    cli = ['--synthetic', '40', '32', '32', '--fps', '10', '--lr_window', '1', '-c', '1', '-b', '2', '--suffix', 'irnbf16',
           '-a', 'IRN', '--precision', 'bf16']
    main.main(['train'] + cli + ['-e', '2', '--save_iter', '1', '-p', '1', '-w', wd])
    ckpts = sorted(glob.glob(os.path.join(wd, 'train', '*', 'checkpoints', 'epoch=*.ckpt')))
    assert [os.path.basename(c) for c in ckpts] == ['epoch=0.ckpt', 'epoch=1.ckpt']
    ck1 = load_checkpoint(ckpts[1], map_location='cpu')
    assert all(torch.isfinite(v).all() for v in ck1['state_dict'].values() if v.is_floating_point())
    main.main(['train'] + cli + ['-e', '3', '--save_iter', '1', '-p', '5', '-w', wd, '-r', ckpts[1]])
    ck2 = load_checkpoint(os.path.join(os.path.dirname(ckpts[1]), 'epoch=2.ckpt'), map_location='cpu')
    assert ck2['epoch'] == 2 and ck2['global_step'] == 3
    frames = str(tmp_path / 'frames')
    main.main(['test'] + cli + ['-w', wd, '-r', ckpts[1], '--save_images', frames])
    assert len(os.listdir(frames)) == 18
