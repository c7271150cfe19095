"""Training with a feature branch switched off (use_1d_feature / use_2d_feature / use_3d_feature) on the HOST build of the unchanged kernel sources
(tests/hipcpu): the `check_*` bodies below are shared with tests/test_gpu_branch_backward.py, which runs them on the MI355X.

1. the masked tap scatter (sherf_gather_tokens_bwd_masked, csrc/gather.hip) on the synthetic scenes of tests/test_hipcpu_gather_edges.py against that
   suite's float64 `ref_backward`, at its standing bound;
2. whole training steps against recorded gradients of the UNMODIFIED reference built with the same switches
   (tools/make_golden_branch_grad.py -> tests/golden/grad_tiny_ri_*f<abc>.npz), both decoders, with and without the transformer;
3. the BatchNorm running statistics follow the constructor's use_3d_feature; 4. the degenerate switch combinations; 5. which entry points a step calls.
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import sherf_oracle as O
from sherf_amd import _lib
from tests import gpu_common as G
from tests import test_hipcpu_gather_edges as E
from tests import test_hipcpu_osg as OSG
from tests.test_hipcpu_frame import cpu_product          # noqa: F401  (the host builds behind sherf_amd._lib, CPU tensors)
from tests.test_hipcpu_osg_backward import osg_grad_frame as grad_frame      # (a grad-enabled `tiny_ri` forward with the three feature inputs as leaves)

#        golden tag          decoder  use_trans  branches
CASES = {'f110':             ('nerf', True,      (True, True, False)),
         'f101':             ('nerf', True,      (True, False, True)),
         'f011':             ('nerf', True,      (False, True, True)),
         'f100':             ('nerf', True,      (True, False, False)),
         'notrans_f101':     ('nerf', False,     (True, False, True)),
         'osg_notrans_f101': ('osg',  False,     (True, False, True)),
         'osg_f100':         ('osg',  True,      (True, False, False))}
MASK_TABLES = {1: ('planes',), 2: ('feat',), 4: ('rows0', 'rows1', 'rows2')}
EINVAL = -1                                              # SHERF_EINVAL: what SHERF_CHECK_ARG returns


def _sync():
    if not G.CPU_SHIM:
        torch.cuda.synchronize()


# ---- 1. the masked scatter through the C ABI ---------------------------------------------------------------------------------------------------
def _present(mask):
    return [k for bit, names in MASK_TABLES.items() if mask & bit for k in names]


def masked_backward(dev, n, d_tiled, mask, null_absent=False, entry='masked'):
    """sherf_gather_tokens_bwd_masked (or, entry='binned', the all-on entry point) on the first n samples of the scene behind `dev`, the outputs in the
    guard layout of E.Dev.backward: zero-filled tables carved out of one buffer with E.GUARD zeros before, between and behind them.  null_absent: the
    absent branches' tables are not allocated and NULL is passed.  -> ({table: gradient, 'bias'}, guards)"""
    p = _lib.ptr
    shapes = dict(E.table_shapes(dev.sc), bias=(96,))
    if null_absent:
        shapes = {k: s for k, s in shapes.items() if k == 'bias' or k in _present(mask)}
    sizes = [int(np.prod(s)) for s in shapes.values()]
    flat = G.dev_tensor(torch.zeros(sum(sizes) + E.GUARD * (len(sizes) + 1), device=None if G.CPU_SHIM else 'cuda'))
    out, guards, o = {}, [], 0
    for (k, s), size in zip(shapes.items(), sizes):
        guards.append(flat[o:o + E.GUARD])
        out[k] = flat[o + E.GUARD:o + E.GUARD + size].view(s)
        o += E.GUARD + size
    guards.append(flat[o:])
    assert guards[-1].numel() == E.GUARD
    q = lambda k: p(out[k]) if k in out else None
    words = ctypes.c_int64(0)
    _lib.call('sherf_gather_bwd_scratch_words', dev.levels[False], n, ctypes.byref(words))
    scratch = G.dev_tensor(torch.full((words.value + 64,), -7, dtype=torch.int32, device=None if G.CPU_SHIM else 'cuda'))
    cnt = dev.counters(n)                                    # (kept alive across the call)
    args = (p(cnt), p(dev.geom), p(d_tiled), E.P, E.HF, E.WF, E.H, E.W, dev.levels[False], p(dev.bounds), p(dev.vox_min), dev.vox_sh, n,
            q('planes'), q('feat'), q('rows0'), q('rows1'), q('rows2'), q('bias'), p(scratch), words.value)
    if entry == 'binned':
        with E.experiment(0):
            _lib.call('sherf_gather_tokens_bwd_binned', *args, _lib.stream())
            _sync()
    else:
        _lib.call('sherf_gather_tokens_bwd_masked', *args, mask, _lib.stream())
        _sync()
    assert bool((scratch[words.value:] == -7).all()), (mask, 'the scratch was written behind its end')
    return out, guards


def assert_masked(sc, label, out, guards, n, mask, ref):
    """Present tables and the bias within E.BOUND of float64 (E._err: relative to the table's largest entry); absent tables bit-zero; guards untouched."""
    assert all(bool((G.plain(g).view(torch.int32) == 0).all()) for g in guards), (label, 'a scatter landed outside its table')
    for k in ('planes', 'feat', 'rows0', 'rows1', 'rows2'):
        if k not in out:
            continue
        ours = G.plain(out[k])
        if k in _present(mask):
            if float(ref[k].abs().max()) == 0:
                assert bool((ours == 0).all()), (label, k)
                continue
            e = E._err(ours, ref[k])
            print(f'{label:30s} {k:7s} ours {e:.2e}')
            assert e <= E.BOUND, (label, k, e)
        else:
            assert bool((ours.contiguous().view(torch.int32) == 0).all()), (label, k, 'a table of an absent branch was written')
    e = E._err(G.plain(out['bias']), ref['bias'])
    print(f'{label:30s} {"bias":7s} ours {e:.2e}')
    assert e <= E.BOUND, (label, 'bias', e)


_REFS = {}


def _ref(name, sc, n):
    if (name, n) not in _REFS:
        _REFS[name, n] = E.ref_backward(sc, sc.geom[:n], sc.d_tok[:n], torch.float64)
    return _REFS[name, n]


def check_masked_scatter(n):
    """The small scene's first n samples (1, 33, 65, 200: one lane, a tile and a lane, a chunk and a lane, four chunks), every mask 1..7, once into
    zero-filled tables for all branches and once with NULL for the absent ones; mask 7 against sherf_gather_tokens_bwd_binned."""
    sc, dev = E.scene_on_device('small')
    assert sc.n >= 200
    d_tiled = G.dev_tensor(E.tile_tokens(sc.d_tok[:n], (n + 31) // 32, fill=3.0))
    ref = _ref('small', sc, n)
    for mask in range(1, 8):
        for null_absent in (False, True):
            out, guards = masked_backward(dev, n, d_tiled, mask, null_absent)
            assert_masked(sc, f'n={n} mask={mask}{" NULL" if null_absent else ""}', out, guards, n, mask, ref)
            if mask == 7 and not null_absent:
                binned, _ = masked_backward(dev, n, d_tiled, 7, entry='binned')
                for k, v in binned.items():
                    b = G.plain(v)
                    if float(b.abs().max()) > 0:
                        assert E._err(G.plain(out[k]), b) <= E.BOUND, (n, k)


def check_masked_scatter_long_run():
    """The long-run scene (5000 samples in one finest cell: running sums carried across chunk boundaries and flushed once), masks 3 and 5."""
    sc, dev = E.scene_on_device('run')
    assert sc.groups['run'].numel() == 5000
    n = sc.n
    d_tiled = G.dev_tensor(E.tile_tokens(sc.d_tok, (n + 31) // 32, fill=3.0))
    ref = _ref('run', sc, n)
    for mask in (3, 5):
        out, guards = masked_backward(dev, n, d_tiled, mask)
        assert_masked(sc, f'run n={n} mask={mask}', out, guards, n, mask, ref)


def check_masked_abi():
    """Declared and exported; branches 0 and 8 are argument errors before anything is launched (the tables stay zero); so is NULL for a PRESENT branch."""
    assert 'sherf_gather_tokens_bwd_masked' in _lib.parse_header(_lib.HEADER)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'sherf_gather_tokens_bwd_masked')
    sc, dev = E.scene_on_device('small')
    n = 33
    d_tiled = G.dev_tensor(E.tile_tokens(sc.d_tok[:n], 2, fill=3.0))
    for mask in (0, 8, -1):
        with pytest.raises(RuntimeError, match=rf'sherf_gather_tokens_bwd_masked failed \({EINVAL}\).*bad argument'):
            masked_backward(dev, n, d_tiled, mask)
    l, p = _lib.lib(), _lib.ptr
    t = {k: G.dev_tensor(torch.zeros(s)) for k, s in dict(E.table_shapes(sc), bias=(96,)).items()}
    words = ctypes.c_int64(0)
    _lib.call('sherf_gather_bwd_scratch_words', dev.levels[False], n, ctypes.byref(words))
    scratch = G.dev_tensor(torch.zeros(words.value, dtype=torch.int32))
    cnt = dev.counters(n)
    head = (p(cnt), p(dev.geom), p(d_tiled), E.P, E.HF, E.WF, E.H, E.W, dev.levels[False], p(dev.bounds), p(dev.vox_min), dev.vox_sh, n)
    tabs = [p(t[k]) for k in ('planes', 'feat', 'rows0', 'rows1', 'rows2')]
    for mask, missing in ((1, 0), (2, 1), (4, 2), (4, 4), (7, 0)):
        a = list(tabs)
        a[missing] = None
        assert l.sherf_gather_tokens_bwd_masked(*head, *a, p(t['bias']), p(scratch), words.value, mask, _lib.stream()) == EINVAL, (mask, missing)
        assert b'bad argument' in l.sherf_last_error()
    for mask in (0, 8):
        assert l.sherf_gather_tokens_bwd_masked(*head, *tabs, p(t['bias']), p(scratch), words.value, mask, _lib.stream()) == EINVAL
    _sync()
    assert all(bool((G.plain(v) == 0).all()) for v in t.values())


# ---- 2. the training step against the unmodified reference's gradients ----------------------------------------------------------------------
def modules(kind, use_trans, branches):
    """A fresh (renderer, decoder) pair with the `tiny_ri` weights: the step moves running statistics and leaves .grad behind."""
    if kind == 'osg':
        return OSG.osg_modules('f16x3', use_trans, branches, fresh=True)
    return G._hip_modules.__wrapped__('f16x3', 'ri', use_trans, tuple(branches))


@contextlib.contextmanager
def autograd_on(rend, kind):
    rend.enable_autograd = True
    if kind == 'osg':
        rend.enable_osg_autograd = True
    try:
        yield
    finally:
        del rend.enable_autograd
        if 'enable_osg_autograd' in rend.__dict__:
            del rend.enable_osg_autograd


def _buffers(rend):
    return {k: G.plain(v).clone() for k, v in rend.encoder_3d.named_buffers()}


def _buffers_moved(before, rend):
    after = _buffers(rend)
    same = lambda a, b: torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)) if a.is_floating_point() else torch.equal(a, b)
    return any(not same(after[k], v) for k, v in before.items())


def train_step(kind, use_trans, branches):
    """Forward with autograd on, stub loss, loss.backward() on `tiny_ri` -> dict(loss, grads {name: tensor}, none [names], moved, rend, dec)."""
    rend, dec = modules(kind, use_trans, branches)
    assert (rend.transformer is not None) == use_trans
    before = _buffers(rend)
    with autograd_on(rend, kind):
        rgb, depth, acc, leaves = grad_frame(rend, dec)
        assert rgb.requires_grad and acc.requires_grad and not depth.requires_grad
        assert int(rend.last['ws']['counters'][0]) == 628
        loss = O.stub_loss(rgb[0], acc[0, :, 0])
        loss.backward()
        _sync()
    grads, none = {}, []
    named = list(leaves.items()) + [(pre + name, p_) for mod, pre in ((rend, 'renderer.'), (dec, 'decoder.')) for name, p_ in mod.named_parameters()]
    for name, t in named:
        if t.grad is None:
            none.append(name)
        else:
            assert t.grad.shape == t.shape, name
            grads[name] = G.plain(t.grad).float()
    return dict(loss=float(loss.detach()), grads=grads, none=none, moved=_buffers_moved(before, rend), rend=rend, dec=dec)


def check_training_step(tag):
    """A step of the renderer built with the tag's switches against tests/golden/grad_tiny_ri_<tag>.npz (the shape of
    tests/test_hipcpu_osg_backward.py::check_full_backward): the names with a gradient are the golden's and every name in its `none_names` has
    .grad None, the three leaves included; every gradient within 1e-2 on the norm and 5e-2 on the fingerprint's entries (the bounds of
    tests/test_gpu_backward.py::test_full_backward_against_reference_gradients).  The loss within 1e-3: the image is within 1e-4 of its largest entry
    (tests/test_hipcpu_frame.py::check_feature_branch_switches holds that for these renderers too), so each squared difference moves by at most 4e-4
    and the loss (1.5-1.6) by 5e-4 of itself, as derived in check_full_backward.  The encoder_3d buffers moved iff they did in the reference's step."""
    kind, use_trans, branches = CASES[tag]
    ref = np.load(os.path.join(G.GOLDEN, f'grad_tiny_ri_{tag}.npz'))
    step = train_step(kind, use_trans, branches)
    assert step['rend'].feature_branches() == branches
    e_loss = abs(step['loss'] - float(ref['loss'])) / float(ref['loss'])
    print(f'branch backward {tag}: loss {step["loss"]:.6f} vs the reference\'s {float(ref["loss"]):.6f} ({e_loss:.2e})')
    assert e_loss < 1e-3
    meta = ('loss', 'none_names', 'encoder_3d_buffers_changed')
    names = [k for k in ref.files if k not in meta]
    grads = step['grads']
    assert set(names) == set(grads), set(names) ^ set(grads)
    assert set(str(k) for k in ref['none_names']) == set(step['none']), set(str(k) for k in ref['none_names']) ^ set(step['none'])
    assert step['moved'] == bool(ref['encoder_3d_buffers_changed'])
    worst = [0.0, 0.0, '', '']
    for k in names:
        ours, r = O.grad_fingerprint(grads[k]), ref[k]
        en, ev = abs(ours[2] - r[2]) / (r[2] + 1e-30), np.linalg.norm(ours[3:] - r[3:]) / (np.linalg.norm(r[3:]) + 1e-30)
        if en > worst[0]:
            worst[0], worst[2] = en, k
        if ev > worst[1]:
            worst[1], worst[3] = ev, k
        assert en < 1e-2, (k, ours[2], r[2])
        assert ev < 5e-2, (k, ev)
    print(f'branch backward {tag}: {len(names)} gradients, worst norm error {worst[0]:.3e} ({worst[2]}), worst fingerprint error {worst[1]:.3e} ({worst[3]})')


# ---- 3. BatchNorm buffers -------------------------------------------------------------------------------------------------------------------
def check_running_statistics():
    """A renderer BUILT with use_3d_feature=False (f110) leaves every encoder_3d buffer bit for bit where it was through a grad-recorded forward and its
    backward, as the reference does (renderer.py:345-352; the golden's flag); f101's move."""
    for tag, moved in (('f110', False), ('f101', True)):
        kind, use_trans, branches = CASES[tag]
        assert bool(np.load(os.path.join(G.GOLDEN, f'grad_tiny_ri_{tag}.npz'))['encoder_3d_buffers_changed']) == moved
        assert train_step(kind, use_trans, branches)['moved'] == moved, tag


# ---- 4. degenerate switches -----------------------------------------------------------------------------------------------------------------
def check_degenerate_switches():
    """(False, False, True) has no branch in run_model's chain and trains like (True, False, False): the name set of grad_tiny_ri_f100.npz, every
    gradient within 1e-4 of the (True, False, False) run's (relative to its norm: the same kernels on the same inputs, fp32 atomics in another order)
    -- but its encoder_3d buffers move, since the reference still runs the encoder under use_3d_feature=True."""
    ref = np.load(os.path.join(G.GOLDEN, 'grad_tiny_ri_f100.npz'))
    a = train_step('nerf', True, (True, False, False))
    b = train_step('nerf', True, (False, False, True))
    assert b['rend'].feature_branches() == (True, False, False)
    names = {k for k in ref.files if k not in ('loss', 'none_names', 'encoder_3d_buffers_changed')}
    assert set(b['grads']) == names == set(a['grads']), set(b['grads']) ^ names
    for k in sorted(names):
        e = float((b['grads'][k].double() - a['grads'][k].double()).norm() / a['grads'][k].double().norm())
        assert e < 1e-4, (k, e)
    assert b['moved'] and not a['moved']


# ---- 5. what runs ---------------------------------------------------------------------------------------------------------------------------
ENCODER_BACKWARD = ('sherf_bwd_bn_relu', 'sherf_bwd_conv_wgrad', 'sherf_bwd_conv_dgrad', 'sherf_svox_conv3_dgrad', 'sherf_bwd_gather_rows')


@contextlib.contextmanager
def recorded_calls():
    calls = []
    fwd, bwd = _lib.call, _lib.call_bwd

    def call(name, *a):
        calls.append((name, a))
        return fwd(name, *a)

    def call_bwd(name, *a):
        calls.append((name, a))
        return bwd(name, *a)
    _lib.call, _lib.call_bwd = call, call_bwd
    try:
        yield calls
    finally:
        _lib.call, _lib.call_bwd = fwd, bwd


def check_what_runs():
    """f110: one masked scatter with branches == 3, no all-on scatter, no entry point of the encoder's backward, no BatchNorm recompute of the tapped
    levels; f101: the mask is 5 and the feature map (two groups of 32 channels) is not unfolded; all on: the masked entry is never called."""
    for branches, mask in (((True, True, False), 3), ((True, False, True), 5), ((True, True, True), None)):
        with recorded_calls() as calls:
            train_step('nerf', True, branches)
        names = [c[0] for c in calls]
        masked = [c for c in calls if c[0] == 'sherf_gather_tokens_bwd_masked']
        if mask is None:
            assert not masked and names.count('sherf_gather_tokens_bwd_binned') == 1
            continue
        assert len(masked) == 1 and masked[0][1][-2] == mask and 'sherf_gather_tokens_bwd_binned' not in names, (branches, len(masked))
        unfolds = [c[1][4] for c in calls if c[0] == 'sherf_bwd_unfold32']             # `groups`: 3 = the tri-planes, 2 = the feature map
        if mask == 3:
            assert not [n for n in names if n in ENCODER_BACKWARD + ('sherf_bwd_bn_relu_apply',)], [n for n in names if n in ENCODER_BACKWARD]
            assert unfolds == [3, 2]
            a = masked[0][1]
            assert a[13] is not None and a[14] is not None and a[15] is None and a[16] is None and a[17] is None      # the voxel rows: NULL
        else:
            assert unfolds == [3] and 'sherf_bwd_conv_wgrad' in names
            assert masked[0][1][14] is None


# ---- the host build -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 33, 65, 200))
def test_masked_scatter_against_float64(cpu_product, n):
    check_masked_scatter(n)


def test_masked_scatter_long_run(cpu_product):
    check_masked_scatter_long_run()


def test_masked_scatter_abi(cpu_product):
    check_masked_abi()


@pytest.mark.parametrize('tag', list(CASES))
def test_branch_training_step_against_reference_gradients(cpu_product, tag):
    check_training_step(tag)


def test_running_statistics_follow_the_constructor_switch(cpu_product):
    check_running_statistics()


def test_degenerate_switches_train_like_planes_alone(cpu_product):
    check_degenerate_switches()


def test_what_a_branch_step_runs(cpu_product):
    check_what_runs()
