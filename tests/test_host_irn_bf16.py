"""Host-side checks of the IRN mixed-precision path (no GPU): the sininn_dense_bf16_args guards refuse a bad call before
anything is launched (pointers are never dereferenced), and `-a IRN --precision bf16` constructs."""
import ctypes as C
import types

import pytest


def _lib():
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib
    return _lib, _lib.lib()


FAKE = 0x7f0000000000                      # 16-byte aligned, never dereferenced on the host


def _pad8(n):
    return (n + 7) // 8 * 8


def _pad16(n):
    return (n + 15) // 16 * 16


def _args(L, b=2, h=8, w=8, cin=12, cout=20, mode=2, **over):
    m = b * h * w
    cinp = _pad8(cin)
    bw = cinp + 128
    a = L.DenseBf16Args(B=b, H=h, W=w, cin=cin, cout=cout, mode=mode, clamp=1.0)
    a.x, a.x_stride, a.aux1, a.aux1_stride, a.aux2, a.buf, a.out = FAKE, cin, FAKE, cout, FAKE, FAKE, FAKE
    for i in range(5):
        a.w_fwd[i] = a.b_fwd[i] = a.w_dgrad[i] = FAKE
        np_ = 32 if i < 4 else _pad16(_pad8(cout))
        kin = cinp + 32 * i
        a.w_fwd_elems[i], a.b_fwd_floats[i] = 9 * np_ * _pad16(kin), np_
        a.w_dgrad_elems[i] = 9 * _pad16(kin) * (32 if i < 4 else _pad16(_pad8(cout)))
    a.buf_elems, a.out_floats, a.aux2_floats = m * bw, m * cout, m * cout
    a.dout, a.dF, a.dD, a.dh, a.dv, a.workspace = FAKE, FAKE, FAKE, FAKE, FAKE, FAKE
    a.dout_floats, a.dF_floats, a.dD_floats, a.dh_floats, a.dv_floats = m * cout, m * bw, m * _pad8(cout), m * cout, m * cout
    a.workspace_bytes = 1 << 30
    for k, v in over.items():
        if isinstance(v, tuple):                 # (array field, index, value)
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def test_dense_bf16_descriptor_is_size_tagged_and_exported():
    L, lib = _lib()
    assert lib.sininn_sizeof(6) == C.sizeof(L.DenseBf16Args)
    assert lib.sininn_sizeof(2) == C.sizeof(L.DenseArgs)           # the fp32 descriptor is unchanged
    assert lib.sininn_version() == 4
    a = L.DenseBf16Args()
    assert a.struct_bytes == C.sizeof(L.DenseBf16Args) and a.buf_bf16 == 1 and a.w_bf16 == 1
    for name in ('sininn_dense_forward_bf16', 'sininn_dense_backward_bf16', 'sininn_dense_bf16_workspace_bytes',
                 'sininn_pack_batch_bf16', 'sininn_pack_work_items_bf16'):
        assert name in L.EXPORTED and hasattr(lib, name)


@pytest.mark.parametrize('cin,cout', [(24, 24), (108, 84), (84, 108), (12, 180), (180, 12)])
def test_dense_bf16_workspace_covers_every_irn_shape(cin, cout):
    """The five weight-gradient items of every IRN DenseBlock shape plan as one mixed group (conv5's N = 84 / 108 / 12 / 180
    included); the planner returns 0 for a group it refuses."""
    _, lib = _lib()
    assert lib.sininn_dense_bf16_workspace_bytes(2, 64, 64, cin, cout) > 0


def test_dense_bf16_guards_refuse_before_any_launch():
    L, lib = _lib()
    m, cout, bw = 2 * 8 * 8, 20, 16 + 128
    cases = [
        (lib.sininn_dense_forward_bf16, dict(struct_bytes=C.sizeof(L.DenseBf16Args) - 8), b'struct_bytes'),
        (lib.sininn_dense_forward_bf16, dict(struct_bytes=C.sizeof(L.DenseArgs)), b'struct_bytes'),
        (lib.sininn_dense_forward_bf16, dict(buf_bf16=0), b'dtype flags'),
        (lib.sininn_dense_forward_bf16, dict(w_bf16=2), b'dtype flags'),
        (lib.sininn_dense_backward_bf16, dict(buf_bf16=0), b'dtype flags'),
        (lib.sininn_dense_forward_bf16, dict(buf_elems=m * bw - 1), b'buf holds'),
        (lib.sininn_dense_forward_bf16, dict(out_floats=m * cout - 4), b'out holds'),
        (lib.sininn_dense_forward_bf16, dict(aux2_floats=0), b'aux2 holds'),
        (lib.sininn_dense_forward_bf16, dict(w_fwd_elems=(4, 100)), b'pack 4'),
        (lib.sininn_dense_forward_bf16, dict(b_fwd_floats=(0, 16)), b'pack 0'),
        (lib.sininn_dense_backward_bf16, dict(w_dgrad_elems=(2, 9 * 80 * 32 - 1)), b'dgrad pack 2'),
        (lib.sininn_dense_backward_bf16, dict(dF_floats=m * (bw - 8)), b'dF holds'),
        (lib.sininn_dense_backward_bf16, dict(dD_floats=m * cout), b'dD holds'),     # needs pad8(cout) = 24 columns
        (lib.sininn_dense_backward_bf16, dict(dh_floats=m), b'dh / dv hold'),
        (lib.sininn_dense_backward_bf16, dict(dout_floats=m), b'dout holds'),
        (lib.sininn_dense_forward_bf16, dict(cin=10), b'multiples of 4'),
        (lib.sininn_dense_forward_bf16, dict(mode=4), b'mode'),
    ]
    for fn, over, word in cases:
        a = _args(L, **over)
        rc = fn(a, None) if fn is lib.sininn_dense_forward_bf16 else fn(a, None, None)
        assert rc != 0 and word in lib.sininn_last_error(), (over, lib.sininn_last_error())
    # the fp32 entry point refuses the bf16 descriptor's size (and vice versa): the two cannot be confused
    a = L.DenseArgs(B=2, H=8, W=8, cin=12, cout=20, mode=0, winograd=0, clamp=1.0)
    a.struct_bytes = C.sizeof(L.DenseBf16Args)
    assert lib.sininn_dense_forward(a, None) != 0 and b'struct_bytes' in lib.sininn_last_error()


def test_pack_work_items_bf16_layout():
    """bf16 batched pack work = fwd [9][Np][pad16(Cin)] + dgrad [9][Cdp][pad16(N)] + bias [Np]; Winograd descriptors refused."""
    L, lib = _lib()
    d = L.PackDesc()
    d.w, d.N, d.Cin, d.ksize, d.Np, d.Cdp = FAKE, 88, 152, 3, 96, 160
    d.w_fwd, d.b_fwd, d.w_dgrad = FAKE, FAKE, FAKE
    d.src_n, d.gap_begin, d.gap_len = 84, 84, 4
    assert lib.sininn_pack_work_items_bf16(C.byref(d)) == 9 * 96 * 160 + 9 * 160 * 96 + 96
    d.wino_fwd = 1
    assert lib.sininn_pack_work_items_bf16(C.byref(d)) == 0


def test_irn_bf16_constructs_and_propagates():
    """`-a IRN --precision bf16` used to raise NotImplementedError at construction."""
    import lit_wrapper
    opt = types.SimpleNamespace(scale=4, num_coupling=1, lr_window=1, architecture='IRN', gpu_ids=[0], rotation=5.0,
                                translation=5.0, tcr_iters=1, lambda_fwd_rec=1.0, lambda_fwd_mmd=0.0,
                                lambda_latent_nll=0.0, lambda_bwd_rec=1.0, lambda_bwd_mmd=0.0, lambda_bwd_tcr=0.0,
                                learning_rate=1e-4, adam_betas=[0.9, 0.99], weight_decay=1e-5, temp=0.8,
                                operation='train', fps=1, lr_dims=12, z_dims=180, precision='bf16')
    model = lit_wrapper.SingleVideoINN(3, 32, 32, opt)
    blocks = model.inn.dense_blocks()
    assert len(blocks) == 6 and all(b.precision == 'bf16' for b in blocks)
    model.inn.set_precision('fp32')
    assert all(b.precision == 'fp32' for b in blocks)
