"""csrc/composite.hip per ray, on rays built by hand (no rendered frame): the two forward kernels (compact, dense) and the two backward kernels through
the C ABI against a transcription of MipRayMarcher2.run_forward in torch FLOAT64 (`march`), gradients by torch.autograd on a fixed seeded linear loss.

  * The reference reads the kernels' own fp32 inputs widened to fp64: depths near + fl(fl(k / (S - 1)) * fl(far - near)) (rounding for rounding), the
    global clamp range as two fp32 numbers.  The compact kernels get a ray's valid samples; the reference and the dense kernels get the dense [R,S]
    arrays with (rgb 0, sigma -80) in the rejected slots.
  * The transcription is anchored once: in fp64 it reproduces tests/golden/marcher_softplus.npz (the UNMODIFIED reference's recorded outputs and
    gradients) at the bounds the suite already holds the kernels to on that golden.
  * Errors are measured PER RAY.  Outputs: absolute (weights sum to <= 1; depth on rays with acc > ACC_FLOOR).  Gradients: max_k |g - ref| over the
    ray's samples divided by max_k |ref|; a ray whose reference maximum is exactly 0 must be exactly 0.
  * The bound of a (case class, quantity) is 4 x the error of the SAME transcription run in float32 on the CPU (FP32_REF_ERR below, measured once by
    `fp32_reference_errors` and written down; DESIGN.md holds the table), with a floor of four fp32 ulps of the quantity's scale.  No bound comes
    from a kernel's output.
  * Discrete facts are asserted exactly: empty rays, relu's sigma <= 0 mask, d_colors == g_c w, compact == dense and BATCH 1 == BATCH 4 bit for bit,
    the capacity branch of sherf_composite_compact_cap, the refusals.

Every output buffer starts filled with a sentinel and has guard rows behind it; sample_out / cs_idx have exactly the rows a call may read, then NaN /
sentinel guard rows (a read behind the end poisons a rendered ray).  The `check_*` bodies run on the HOST build of the unchanged kernel sources below and
on the MI355X in tests/test_gpu_composite_edges.py."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from sherf_amd import _lib
from tests import gpu_common as G
from tests.test_hipcpu_frame import cpu_product          # noqa: F401  (the host builds behind sherf_amd._lib, CPU tensors)
from tests.test_hipcpu_gather_edges import _sync, experiment
from tests.test_hipcpu_sampler_edges import _full, f2ord
from tests.test_hipcpu_softplus import CASES as GOLDEN_CASES, _depths_like_the_kernel, _expected_grad, _marcher_golden

F = np.float32
SENT, FSENT, GUARD = -1234567, -7.5, 64
MODES = ('relu', 'softplus')
ULP = 2.0 ** -23
FLT_MIN = 2.0 ** -126
ACC_FLOOR = 1e-3                                         # depth = D / W: its error grows as 1 / acc; rays below this are compared on rgb / acc / w alone
QUANTITIES = ('rgb', 'acc', 'w', 'depth', 'd_colors', 'd_sigma', 'c_rgb', 'c_sigma')
# four fp32 ulps of the quantity's scale: rgb spans [-1, 1] (ulp of 2), acc and w [0, 1], depth the largest depth of a case (< 4), gradients relative
FLOOR = dict(rgb=8 * ULP, acc=4 * ULP, w=4 * ULP, depth=16 * ULP, d_colors=4 * ULP, d_sigma=4 * ULP, c_rgb=4 * ULP, c_sigma=4 * ULP)
FACTOR = 4.0                                             # a device expf / log1pf of 1-2 ulp, sequential sums where torch uses cumprod; nothing else differs

# The per-ray error of `march` in float32 (torch, CPU) against `march` in float64, worst ray of every case of the class, both clamp modes, white_back
# both ways (fp32_reference_errors; python -m tests.test_hipcpu_composite_edges prints this table).  d_colors / d_sigma: the dense kernels' loss
# (rgb, depth, w), c_rgb / c_sigma: the compact kernels' (rgb, acc).
FP32_REF_ERR = {
    'counts': dict(rgb=4.16e-07, acc=1.25e-07, w=8.78e-08, depth=6.91e-07, d_colors=4.46e-07, d_sigma=4.61e-04, c_rgb=4.46e-07, c_sigma=1.25e-05),
    'zero_neg': dict(rgb=2.87e-07, acc=6.00e-08, w=6.77e-08, depth=3.11e-07, d_colors=1.05e-07, d_sigma=3.25e-07, c_rgb=1.05e-07, c_sigma=3.18e-06),
    'last_tiny': dict(rgb=4.07e-07, acc=1.19e-07, w=4.80e-08, depth=1.40e-07, d_colors=5.91e-07, d_sigma=3.70e-04, c_rgb=5.91e-07, c_sigma=1.01e-06),
    'opaque': dict(rgb=2.37e-07, acc=5.99e-08, w=5.30e-08, depth=1.64e-07, d_colors=1.39e-07, d_sigma=1.34e-06, c_rgb=1.39e-07, c_sigma=1.50e-06),
    'threshold': dict(rgb=2.77e-07, acc=1.15e-07, w=9.25e-08, depth=1.88e-07, d_colors=3.96e-07, d_sigma=5.10e-07, c_rgb=3.96e-07, c_sigma=4.53e-07),
    'scale': dict(rgb=3.15e-07, acc=6.00e-08, w=5.40e-08, depth=3.25e-07, d_colors=1.12e-07, d_sigma=2.87e-07, c_rgb=1.12e-07, c_sigma=3.44e-07),
    'clamped': dict(rgb=3.33e-07, acc=1.19e-07, w=5.93e-08, depth=2.47e-07, d_colors=1.64e-07, d_sigma=1.38e-06, c_rgb=1.64e-07, c_sigma=5.93e-07),
}


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------------------------------
def march(colors, sigma, t, rd, mode, white_back, lo, hi):
    """MipRayMarcher2.run_forward on [R,S,3], [R,S], [R,S], [R,3] in the dtype of its inputs; `lo`, `hi`: the global clamp range (the reference takes
    min / max of its depths).  -> rgb [R,3], depth [R], weights [R,S]"""
    delta = torch.cat([t[:, 1:] - t[:, :-1], torch.full_like(t[:, :1], 1e10)], 1) * torch.norm(rd, dim=-1, keepdim=True)
    if mode == 'softplus':
        dens = Fn.softplus(sigma - 1)
    elif mode == 'relu':
        dens = Fn.relu(sigma)
    else:
        raise AssertionError(mode)
    alpha = 1 - torch.exp(-(dens * delta))
    shifted = torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha + 1e-10], 1)
    w = alpha * torch.cumprod(shifted, 1)[:, :-1]
    rgb = torch.sum(w[..., None] * colors, 1)
    total = w.sum(1)
    depth = torch.sum(w * t, 1) / total
    depth = torch.nan_to_num(depth, float('inf'))
    depth = torch.clamp(depth, lo, hi)
    if white_back:
        rgb = rgb + 1 - total[:, None]
    return rgb * 2 - 1, depth, w


def _finite_or(full, fallback):
    return torch.where(torch.isfinite(full), full, fallback)


def reference(case, mode, wb, dtype):
    """`march` in `dtype` on the case's fp32 inputs + autograd of the two fixed losses.  Empty rays keep _expected_grad's contract: where autograd's
    quotient makes 0 / 0 of the zero upstream gradient of a replaced depth, the expected value is the gradient of the loss without its depth term."""
    c, s = case.colors.to(dtype).requires_grad_(True), case.sigma.to(dtype).requires_grad_(True)
    rgb, dep, w = march(c, s, case.t.to(dtype), case.rd.to(dtype), mode, wb, case.lo, case.hi)
    acc = w.sum(1)
    g = {k: v.to(dtype) for k, v in case.g.items()}
    l_compact = (rgb * g['rgb']).sum() + (acc * g['acc']).sum()
    l_nodepth = (rgb * g['rgb']).sum() + (w * g['w']).sum()          # (g['w'] carries the acc term: acc is the sum of the weights)
    l_dense = l_nodepth + (dep * g['depth']).sum()
    grad = lambda l: torch.autograd.grad(l, (c, s), retain_graph=True)
    (cc, cs), (nc, ns), (dc, ds) = grad(l_compact), grad(l_nodepth), grad(l_dense)
    return dict(rgb=rgb.detach(), acc=acc.detach(), depth=dep.detach(), w=w.detach(), d_colors=_finite_or(dc, nc), d_sigma=_finite_or(ds, ns), c_rgb=cc, c_sigma=cs,
                n_dropped=int((~torch.isfinite(ds)).any(1).sum()))


# ---- 2. the cases: rays built by hand ---------------------------------------------------------------------------------------------------------------------
class Rays:
    """One case: rays of S samples, added one by one.  `valid`: the sample indices the shell mask kept; `sigma`: raw values [S] (None: moderate, optical
    depths of order one with zeros and negatives sprinkled in); `empty`: the clamp modes under which the ray is empty by construction."""

    def __init__(self, name, cls, S, seed, clamp=None):
        self.name, self.cls, self.S, self.rs, self.clamp, self.rows = name, cls, S, np.random.RandomState(seed), clamp, []

    def add(self, valid, sigma=None, scale=1.0, span=None, flat=False, zero_d=False, empty=(), mix=True):
        rs, S = self.rs, self.S
        v = np.zeros(S, bool)
        v[list(valid)] = True
        near = rs.uniform(1, 2)
        far = near if flat else near + (rs.uniform(0.5, 2) if span is None else span)
        d = rs.normal(size=3)
        d = np.zeros(3) if zero_d else d / np.linalg.norm(d) * scale
        if sigma is None:
            delta = 1.0 if flat or zero_d else (far - near) / max(S - 1, 1) * scale
            sigma = rs.uniform(0.05, 1.5, S) * 4 / max(4, int(v.sum())) / delta
            if mix and v.sum() > 2:                     # (negatives of a size softplus still sees: no ray whose alpha underflows in fp32 alone)
                u = rs.uniform(size=S)
                sigma = np.where(u < 0.1, 0.0, np.where(u < 0.25, -rs.uniform(0.1, 2, S), sigma))
        if not v.any():
            empty = MODES
        sg = np.where(v, np.broadcast_to(np.asarray(sigma, np.float64), (S,)), -80.0)
        col = np.where(v[:, None], rs.uniform(0, 1, (S, 3)), 0.0)
        self.rows.append((v, sg, col, near, far, d, frozenset(empty), flat or zero_d))
        return len(self.rows) - 1

    def done(self):
        S, rs = self.S, self.rs
        v, sg, col, near, far, d, empty, still = zip(*self.rows)
        tt = lambda a, dt=F: torch.from_numpy(np.ascontiguousarray(np.array(a).astype(dt)))
        c = SimpleNamespace(name=self.name, cls=self.cls, R=len(v), S=S, valid=tt(v, bool), sigma=tt(sg), colors=tt(col), near=tt(near), far=tt(far), rd=tt(d),
                            empty={m: torch.tensor([m in e for e in empty]) for m in MODES})
        # relu: a ray is empty iff no sample with a non-zero delta has sigma > 0 (near == far / the zero direction leave the last sample alone)
        lit = np.array(sg) > 0
        lit[np.array(still), :-1] = False
        lit[np.array([not np.any(x) for x in d])] = False
        c.empty['relu'] = c.empty['relu'] | torch.from_numpy(~lit.any(1))
        c.t = _depths_like_the_kernel(c.near, c.far, S) if S > 1 else c.near[:, None].clone()
        if self.clamp is None:
            c.lo, c.hi = float(c.t.min()), float(c.t.max())
        else:                                            # the clamp range narrowed, as check_dense_backward does
            c.lo, c.hi = (float(c.t.flatten().quantile(q)) for q in self.clamp)
            c.lo, c.hi = float(F(c.lo)), float(F(c.hi))
        R = c.R
        c.g = dict(rgb=tt(rs.normal(size=(R, 3))), acc=tt(rs.normal(size=R)), depth=tt(rs.normal(size=R)))
        c.g['w'] = tt(rs.normal(size=(R, S))) + c.g['acc'][:, None]
        # the compact form
        c.cnt = c.valid.sum(1).to(torch.int32)
        c.base = (torch.cumsum(c.cnt, 0) - c.cnt).to(torch.int32)
        c.idx = torch.nonzero(c.valid.reshape(-1))[:, 0].to(torch.int32)
        c.nv = int(c.idx.numel())
        c.so = torch.cat([c.colors.reshape(-1, 3), c.sigma.reshape(-1, 1)], 1)[c.idx.long()].contiguous()
        return c


def _counts_case(S):
    """ray_cnt in {0, 1, 2, 3, 4, 5, 7, 8, 9, S} (those <= S): the first n, the last n (includes S - 1), n that stop short of S - 1; {0}, {S - 1}, every other"""
    b = Rays(f'counts_S{S}', 'counts', S, 10 + S)
    for n in sorted({0, 1, 2, 3, 4, 5, 7, 8, 9, S}):
        if n > S:
            continue
        b.add(range(n), empty=MODES if n == 0 else ())
        if n:
            b.add(range(S - n, S))
        if 0 < n < S:
            b.add(sorted(b.rs.choice(S - 1, n, replace=False).tolist()))
    b.add([0]); b.add([S - 1]); b.add(range(0, S, 2)); b.add(range(1, S, 2))
    b.add([S - 1], mix=False); b.add(range(S), mix=False); b.add(range(S - 1), mix=False)
    return b.done()


def _dense_S1_case():
    b = Rays('dense_S1', 'counts', 1, 7)
    for i in range(6):
        b.add([0], sigma=[(-80.0, 0.0, 1e-11, 3.0, -2.0, 30.0)[i]], empty=(MODES if i == 0 else ('relu',) if i in (1, 4) else ()))
    return b.done()


def _R_case(R, kind=None):
    """R rays of S = 5 with ragged counts; an empty and a full ray on both sides of every edge of a 256-thread block"""
    S = 5
    b = Rays(f'rays_R{R}{kind or ""}', 'counts', S, 100 + R + (kind == 'empty'))
    edge = {0: 'full', 254: 'empty', 255: 'empty', 256: 'full', 511: 'full', 512: 'empty'}
    if kind:
        edge = {0: kind}
    for r in range(R):
        e = edge.get(r)
        if e == 'empty':
            b.add([], empty=MODES)
        elif e == 'full':
            b.add(range(S), mix=False)
        else:
            b.add(np.flatnonzero(b.rs.uniform(size=S) < 0.6).tolist())
    return b.done()


def _zero_neg_case():
    S = 5
    b = Rays('zero_neg', 'zero_neg', S, 31)
    for i in range(3):
        b.add(range(S), sigma=np.zeros(S), empty=('relu',))
        b.add(range(S), sigma=b.rs.uniform(-15, -0.1, S), empty=('relu',))
        b.add(range(S), sigma=np.full(S, -80.0), empty=MODES)
        b.add([], empty=MODES)
        r = b.add(range(S), mix=False)
        b.rows[r][1][1], b.rows[r][1][2 + i % 2] = 0.0, -3.0          # a zero and a negative among moderate samples
    return b.done()


def _last_tiny_case():
    """1e-12 on the last sample only: the 1e10 delta makes it count under relu (alpha = 1 - exp(-0.01 |d|))"""
    S = 5
    b = Rays('last_tiny', 'last_tiny', S, 32)
    for other in (0.0, -30.0, -80.0):
        for i in range(2):
            b.add(range(S), sigma=np.array([other] * (S - 1) + [1e-12]))
    for i in range(3):
        r = b.add(range(S), mix=False)
        b.rows[r][1][S - 1] = 1e-12
    return b.done()


def _opaque_case():
    """sigma = 1e4: alpha == 1 exactly in fp32, first, in the middle, last, and all three (at most three per ray: T stays a normal fp32 number)"""
    S = 5
    b = Rays('opaque', 'opaque', S, 33)
    for where in ((0,), (2,), (4,), (0, 2, 4), (1, 2)):
        for i in range(3):
            r = b.add(range(S), mix=False)
            for k in where:
                b.rows[r][1][k] = 1e4
    c = b.done()
    c.opaque = c.sigma == 1e4
    return c


THRESHOLD_SIGMAS = (float(np.nextafter(F(21), F(0))), 21.0, float(np.nextafter(F(21), F(99))), 91.0)


def _threshold_case():
    """softplus at sigma - 1 just below, at and just above F.softplus's threshold 20, and at 90 (expf overflows beyond 88.7); thin slabs (delta = 0.005) so
    that alpha is not saturated before the last sample"""
    S = 5
    b = Rays('threshold', 'threshold', S, 34)
    for sg in THRESHOLD_SIGMAS:
        b.add(range(S), sigma=np.full(S, sg), span=0.02)
        b.add(range(S - 1), sigma=np.full(S, sg), span=0.02)
    b.add(range(S), sigma=np.array(THRESHOLD_SIGMAS + (-1.0,)), span=0.02)
    b.add(range(S), sigma=np.array((-1.0,) + THRESHOLD_SIGMAS[::-1]), span=0.02)
    return b.done()


def _scale_case():
    """|d| in {1e-3, 1, 1e3} with the same raw densities, the zero direction, near == far"""
    S = 5
    b = Rays('scale', 'scale', S, 35)
    for scale in (1e-3, 1.0, 1e3):
        for i in range(3):
            b.add(range(S) if i < 2 or scale < 1 else range(S - 1), sigma=b.rs.uniform(0.2, 6, S), scale=scale)
    b.add(range(S), sigma=b.rs.uniform(0.2, 6, S), zero_d=True, empty=MODES)
    b.add(range(S), sigma=b.rs.uniform(0.2, 6, S), flat=True)                                            # near == far: all the weight on the last sample
    b.add(range(S), sigma=np.array([1.0, 2.0, 3.0, 4.0, -80.0]), flat=True, empty=MODES)                  # ... and nothing on it
    b.add(range(S), sigma=np.array([1.0, 2.0, 3.0, 4.0, 0.0]), flat=True, empty=('relu',))
    return b.done()


def _clamped_case():
    S = 5
    b = Rays('clamped', 'clamped', S, 36, clamp=(0.35, 0.65))
    for i in range(24):
        b.add(range(S) if i % 3 else range(S - 1 - i % 2), mix=i % 2 == 0)
    b.add([], empty=MODES)
    return b.done()


CASE_BUILDERS = {**{f'counts_S{S}': functools.partial(_counts_case, S) for S in (2, 3, 5, 64, 65)}, 'dense_S1': _dense_S1_case,
                 'rays_R1full': functools.partial(_R_case, 1, 'full'), 'rays_R1empty': functools.partial(_R_case, 1, 'empty'),
                 **{f'rays_R{R}': functools.partial(_R_case, R) for R in (255, 256, 257, 513)},
                 'zero_neg': _zero_neg_case, 'last_tiny': _last_tiny_case, 'opaque': _opaque_case, 'threshold': _threshold_case, 'scale': _scale_case,
                 'clamped': _clamped_case}
CASE_NAMES = tuple(CASE_BUILDERS)


@functools.lru_cache(None)
def case(name):
    return CASE_BUILDERS[name]()


@functools.lru_cache(None)
def ref64(name, mode, wb):
    """computed once, shared by the host and the device tests, never changed"""
    return reference(case(name), mode, wb, torch.float64)


# ---- 3. the kernels through the C ABI -------------------------------------------------------------------------------------------------------------------
def _guarded(x, fill):
    """x on the device with GUARD rows of `fill` behind it"""
    pad = torch.full((GUARD,) + tuple(x.shape[1:]), fill, dtype=x.dtype)
    return G.dev_tensor(torch.cat([x, pad]).contiguous())


def _take(buf, rows, fill, what):
    b = G.plain(buf)
    tail = b[rows:]
    assert bool((tail == fill).all()) if fill == fill else bool(torch.isnan(tail).all()), f'{what}: written behind its last row'
    return b[:rows]


def _bits(a):
    return a.contiguous().view(torch.int32)


def run_dense(c, mode, wb):
    P, R, S = _lib.ptr, c.R, c.S
    bits = _lib.composite_bits(bool(wb), mode)
    col, sig, t, rd, dmm = (G.dev_tensor(x.contiguous()) for x in (c.colors, c.sigma, c.t, c.rd, torch.tensor([c.lo, c.hi])))
    f32 = torch.float32
    rgb, dep, w = _full((R + GUARD, 3), FSENT, f32), _full(R + GUARD, FSENT, f32), _full((R + GUARD, S), FSENT, f32)
    _lib.call('sherf_composite_dense', P(col), P(sig), P(t), P(rd), R, S, bits, P(dmm), P(rgb), P(dep), P(w), _lib.stream())
    dc, ds = _full((R + GUARD, S, 3), FSENT, f32), _full((R + GUARD, S), FSENT, f32)
    g = {k: G.dev_tensor(v.contiguous()) for k, v in c.g.items()}
    _lib.call('sherf_composite_dense_bwd', P(col), P(sig), P(t), P(rd), R, S, bits, P(dmm), P(g['rgb']), P(g['depth']), P(g['w']), P(dc), P(ds), _lib.stream())
    _sync()
    o = dict(rgb=_take(rgb, R, FSENT, 'rgb'), depth=_take(dep, R, FSENT, 'depth'), w=_take(w, R, FSENT, 'w'), d_colors=_take(dc, R, FSENT, 'd_colors'),
             d_sigma=_take(ds, R, FSENT, 'd_sigma'))
    acc = o['w'][:, 0].clone()
    for k in range(1, S):                                # the kernel's own order of summation
        acc = acc + o['w'][:, k]
    o['acc'] = acc
    return o


def compact_inputs(c, tok_cap=None, flag=0):
    """The compact form of a case on the device: sample_out / cs_idx with exactly `tok_cap` rows (default: the count), NaN / sentinel guard rows behind"""
    rows = c.nv if tok_cap is None else tok_cap
    i = SimpleNamespace(tok_cap=max(rows, 1))
    i.counters0 = torch.tensor([c.nv, f2ord(c.lo), f2ord(c.hi), flag], dtype=torch.int32)
    i.counters = _guarded(i.counters0, SENT)
    i.base, i.cnt = G.dev_tensor(c.base.clone()), G.dev_tensor(c.cnt.clone())
    i.idx, i.so = _guarded(c.idx[:rows], SENT), _guarded(c.so[:rows], float('nan'))
    i.rd, i.near, i.far = (G.dev_tensor(x.contiguous()) for x in (c.rd, c.near, c.far))
    return i


def run_compact_forward(c, i, mode, wb, entry='cap', batch1=False):
    P, R, S, f32 = _lib.ptr, c.R, c.S, torch.float32
    bits = _lib.composite_bits(bool(wb), mode)
    rgb, dep, acc = _full((R + GUARD, 3), FSENT, f32), _full(R + GUARD, FSENT, f32), _full(R + GUARD, FSENT, f32)
    head = (P(i.counters), P(i.base), P(i.cnt), P(i.idx), P(i.so), P(i.rd), P(i.near), P(i.far), R, S, bits)
    with experiment((1 << 20) if batch1 else 0):
        if entry == 'cap':
            _lib.call('sherf_composite_compact_cap', *head, i.tok_cap, P(rgb), P(dep), P(acc), _lib.stream())
        else:
            _lib.call('sherf_composite_compact', *head, P(rgb), P(dep), P(acc), _lib.stream())
        _sync()
    return dict(rgb=_take(rgb, R, FSENT, 'rgb'), depth=_take(dep, R, FSENT, 'depth'), acc=_take(acc, R, FSENT, 'acc'), counters=G.plain(i.counters))


def run_compact_backward(c, i, mode, wb):
    """-> d_sample_out [nv,4] scattered into the dense [R,S,3] / [R,S] layout (zeros in the rejected slots) and the rows themselves"""
    P, R, S = _lib.ptr, c.R, c.S
    assert i.tok_cap >= c.nv                              # never a ray beyond its buffers
    out = _full((c.nv + GUARD, 4), FSENT, torch.float32)
    g_rgb, g_acc = G.dev_tensor(c.g['rgb'].contiguous()), G.dev_tensor(c.g['acc'].contiguous())
    _lib.call('sherf_composite_compact_bwd', P(i.base), P(i.cnt), P(i.idx), P(i.so), P(i.rd), P(i.near), P(i.far), R, S, _lib.composite_bits(bool(wb), mode),
              P(g_rgb), P(g_acc), P(out), _lib.stream())
    _sync()
    rows = _take(out, c.nv, FSENT, 'd_sample_out')
    dc, ds = torch.zeros(R * S, 3), torch.zeros(R * S)
    dc[c.idx.long()], ds[c.idx.long()] = rows[:, :3], rows[:, 3]
    return dict(c_rgb=dc.view(R, S, 3), c_sigma=ds.view(R, S), rows=rows)


# ---- 4. the per-ray error measure ---------------------------------------------------------------------------------------------------------------------------
def _ray_abs(a, ref):
    return (a.double() - ref.double()).abs().reshape(a.shape[0], -1).amax(1)


def _ray_rel(g, ref, mask, what):
    """max_k |g - ref| / max_k |ref| over the samples of `mask` [R,S]; rays whose reference maximum is exactly 0 must be exactly 0, and rays whose reference
    maximum lies below the smallest normal fp32 number (a ray saturated throughout: 1e-139 in fp64) must stay below it"""
    R = g.shape[0]
    m = mask.reshape(R, mask.shape[1], *([1] * (g.dim() - 2))).expand_as(g)
    zero = torch.zeros((), dtype=torch.float64)
    num = torch.where(m, (g.double() - ref.double()).abs(), zero).reshape(R, -1).amax(1)
    den = torch.where(m, ref.double().abs(), zero).reshape(R, -1).amax(1)
    dead = den < FLT_MIN
    mine = torch.where(m, g.double(), zero).abs().reshape(R, -1).amax(1)
    assert bool((mine[den == 0] == 0).all()), f'{what}: a ray whose reference gradient is exactly 0 took one'
    assert bool((mine[dead] <= FLT_MIN).all()), f'{what}: a ray whose reference gradient is below the fp32 range took one'
    return torch.where(dead, zero, num / torch.where(dead, torch.ones_like(den), den))


def ray_errors(c, out, ref):
    """quantity -> [R] per-ray error of `out` (a kernel's results, or the fp32 run of the transcription) against the fp64 reference"""
    every = torch.ones(c.R, c.S, dtype=torch.bool)
    e = {q: _ray_abs(out[q], ref[q]) for q in ('rgb', 'acc', 'w') if q in out}
    e['depth'] = torch.where(ref['acc'] > ACC_FLOOR, _ray_abs(out['depth'], ref['depth']), torch.zeros(c.R, dtype=torch.float64))
    for q, m in (('d_colors', every), ('d_sigma', every), ('c_rgb', c.valid), ('c_sigma', c.valid)):
        if q in out:
            e[q] = _ray_rel(out[q], ref[q], m, f'{c.name} {q}')
    return e


def bound(cls, q):
    return max(FACTOR * FP32_REF_ERR[cls][q], FLOOR[q])


def fp32_reference_errors(names=None):
    """class -> quantity -> the worst per-ray error of the float32 run of `march` against its float64 run (how FP32_REF_ERR was measured)"""
    worst = {}
    for name in names or CASE_NAMES:
        c = case(name)
        for mode in MODES:
            for wb in (0, 1):
                e = ray_errors(c, reference(c, mode, wb, torch.float32), ref64(name, mode, wb))
                for q, v in e.items():
                    assert bool(torch.isfinite(v).all()), (name, mode, wb, q)
                    w = worst.setdefault(c.cls, dict.fromkeys(QUANTITIES, 0.0))
                    w[q] = max(w[q], float(v.max()))
    return worst


KERNEL_ERR = {}                                          # (host | device, class, quantity) -> the worst per-ray error seen (reported, never used for a bound)


# ---- 5. the checks --------------------------------------------------------------------------------------------------------------------------------------------
def check_transcription_against_golden():
    """`march` against the unmodified reference's recorded fp32 outputs and gradients (tests/golden/marcher_softplus.npz).  In float32 it is the recording's
    own arithmetic: outputs within 2 ulps, gradients within 1e-6 of the largest entry, the same entries 0 / 0.  In float64 it agrees at the bounds the suite
    holds the kernels to on that golden (check_dense_forward: 2e-6 / 1e-6 / 1e-5 absolute; check_dense_backward: 1e-5 / 2e-4 of the largest entry) -- the
    fp32 rounding of the golden -- on every ray but the few whose alpha underflows in fp32 alone (0 < acc < ACC_FLOOR in fp64: the recording calls them
    empty, their depth and its gradient have no fp32 counterpart)."""
    g = _marcher_golden()
    for tag in GOLDEN_CASES:
        col, sig, t, rd = (torch.from_numpy(g[tag + k])[0] for k in ('colors', 'dens', 'depths', 'rd'))
        sig, t = sig[..., 0], t[..., 0]
        lo, hi = float(t.min()), float(t.max())
        for wb in (0, 1):
            for mode in MODES:
                for dt in (torch.float32, torch.float64):
                    exact = dt == torch.float32
                    c, s = col.to(dt).requires_grad_(True), sig.to(dt).requires_grad_(True)
                    rgb, dep, w = march(c, s, t.to(dt), rd.to(dt), mode, wb, lo, hi)
                    acc = w.sum(1).detach()
                    ok = torch.ones_like(acc, dtype=torch.bool) if exact else (acc == 0) | (acc > ACC_FLOOR)
                    assert int((~ok).sum()) < ok.numel() // 10
                    if mode == 'softplus':
                        near = lambda a, key, tol: bool(((a.detach().double() - torch.from_numpy(g[f'{tag}{key}_{wb}'])[0].double().reshape(a.shape)).abs()[ok] <= tol).all())
                        assert near(rgb, 'rgb', 2 * ULP if exact else 2e-6) and near(w, 'w', 2 * ULP if exact else 1e-6), (tag, wb, dt)
                        assert near(dep, 'depth', 8 * ULP if exact else 1e-5), (tag, wb, dt)
                    gg = {k: torch.from_numpy(g[tag + 'g_' + k])[0].to(dt) for k in ('rgb', 'depth', 'w')}
                    nodepth = (rgb * gg['rgb']).sum() + (w * gg['w'][..., 0]).sum()
                    full = nodepth + (dep * gg['depth'][:, 0]).sum()
                    (dc, ds), (nc, ns) = torch.autograd.grad(full, (c, s), retain_graph=True), torch.autograd.grad(nodepth, (c, s))
                    ec, _ = _expected_grad(g, f'{tag}d_colors_{mode}_{wb}')
                    es, k = _expected_grad(g, f'{tag}d_dens_{mode}_{wb}')
                    e_c, e_s = G.rel(_finite_or(dc, nc)[ok], ec[0][ok]), G.rel(_finite_or(ds, ns)[ok], es[0, ..., 0][ok])
                    assert e_c < (1e-6 if exact else 1e-5) and e_s < (1e-6 if exact else 2e-4), (tag, mode, wb, dt, e_c, e_s, k)
                    if exact:
                        assert int((~torch.isfinite(ds)).sum()) == k               # the same entries are 0 / 0 in the transcription and in the recording


def _assert_preconditions(c, mode, wb, ref):
    """What a case is there for, from its inputs and the fp64 reference alone (before any kernel runs)"""
    empty = c.empty[mode]
    assert bool((ref['acc'][empty] < 1e-20).all()), (c.name, mode, 'a ray flagged empty is not')
    assert bool((ref['acc'][~empty] > 1e-4).all()), (c.name, mode, 'a ray is neither empty nor far above the underflow of alpha in fp32', ref['acc'])
    assert ref['n_dropped'] <= int(empty.sum())           # (the 0 / 0 of a replaced depth: on empty rays only; relu's backward selects 0 at sigma <= 0)
    if c.cls == 'opaque':
        dn = torch.norm(c.rd, dim=-1, keepdim=True)
        delta = torch.cat([c.t[:, 1:] - c.t[:, :-1], torch.full_like(c.t[:, :1], 1e10)], 1) * dn
        dens = Fn.softplus(c.sigma - 1) if mode == 'softplus' else Fn.relu(c.sigma)
        assert bool(((1 - torch.exp(-(dens * delta)))[c.opaque] == 1).all())       # alpha == 1 exactly in fp32
    if c.cls == 'clamped':
        moved = (ref['depth'] == c.lo) | (ref['depth'] == c.hi)
        assert 4 <= int(moved.sum()) <= c.R - 4, (c.name, int(moved.sum()))
    if c.cls == 'threshold':
        x = c.sigma[c.valid] - 1
        assert bool((x < 20).any()) and bool((x == 20).any()) and bool(((x > 20) & (x < 20.001)).any()) and bool((x == 90).any())


def check_case(name):
    c = case(name)
    where = 'host' if G.CPU_SHIM else 'device'
    S = c.S
    inputs = compact_inputs(c) if S > 1 else None
    for mode in MODES:
        for wb in (0, 1):
            label = (name, mode, wb)
            ref = ref64(name, mode, wb)
            _assert_preconditions(c, mode, wb, ref)
            d = run_dense(c, mode, wb)
            out = dict(d)
            if inputs is not None:
                f4, f1 = run_compact_forward(c, inputs, mode, wb), run_compact_forward(c, inputs, mode, wb, batch1=True)
                plain_entry = run_compact_forward(c, inputs, mode, wb, entry='plain')
                for k in ('rgb', 'depth', 'acc'):
                    assert torch.equal(_bits(f1[k]), _bits(f4[k])), (label, k, 'BATCH = 1 and BATCH = 4 differ')
                    assert torch.equal(_bits(plain_entry[k]), _bits(f4[k])), (label, k, 'sherf_composite_compact and _cap differ')
                    assert torch.equal(_bits(f4[k]), _bits(d[k])), (label, k, 'compact and dense differ on the scattered inputs')
                assert torch.equal(f4['counters'][:4], inputs.counters0) and bool((f4['counters'][4:] == SENT).all()), (label, 'counters')
                b = run_compact_backward(c, inputs, mode, wb)
                out.update(c_rgb=b['c_rgb'], c_sigma=b['c_sigma'])
            # ---- discrete facts ----
            for q in ('d_colors', 'd_sigma', 'c_rgb', 'c_sigma'):
                assert q not in out or bool(torch.isfinite(out[q]).all()), (label, q, 'a gradient is not finite')
            gc = 2 * c.g['rgb']
            assert bool((d['d_colors'] == gc[:, None, :] * d['w'][:, :, None]).all()), (label, 'd_colors != g_c w')
            if inputs is not None:
                assert bool((out['c_rgb'] == torch.where(c.valid[..., None], gc[:, None, :] * d['w'][:, :, None], torch.zeros(()))).all()), (label, 'compact d_rgb != g_c w')
            if mode == 'relu':
                off = c.sigma <= 0
                assert bool((d['d_sigma'][off] == 0).all()) and (inputs is None or bool((out['c_sigma'][off] == 0).all())), (label, 'relu: d_sigma at sigma <= 0')
            empty = c.empty[mode]
            if bool(empty.any()):
                assert bool((d['acc'][empty] == 0).all()) and bool((d['rgb'][empty] == (1.0 if wb else -1.0)).all()), (label, 'empty rays')
                assert torch.equal(_bits(d['depth'][empty]), _bits(torch.full((int(empty.sum()),), c.hi))), (label, 'an empty ray is not at the global maximum depth')
                assert bool((d['w'][empty] == 0).all()) and bool((d['d_colors'][empty] == 0).all()), (label, 'empty rays')
                # d_sigma: exactly 0 where the reference's row is (_ray_rel); under softplus a row of -80 has the derivative z / (z + 1) ~ 6.6e-36, times at most 1e10 |d|
                assert bool((d['d_sigma'][empty].abs() <= (0.0 if mode == 'relu' else 1e-20)).all()), (label, 'empty rays: d_sigma')
            # ---- per ray against fp64 ----
            errs = ray_errors(c, out, ref)
            for q, v in errs.items():
                key = (where, c.cls, q)
                KERNEL_ERR[key] = max(KERNEL_ERR.get(key, 0.0), float(v.max()))
                print(f'{name} {mode} wb={wb} {q}: {float(v.max()):.3e} (bound {bound(c.cls, q):.3e})')
            over = [(q, f'{float(v.max()):.3e}', f'ray {int(v.argmax())}', f'bound {bound(c.cls, q):.3e}') for q, v in errs.items() if not float(v.max()) <= bound(c.cls, q)]
            assert not over, (label, over)
            _class_facts(c, mode, wb, d, out, ref)


def _class_facts(c, mode, wb, d, out, ref):
    label = (c.name, mode, wb)
    if c.cls == 'opaque':
        # behind an exactly opaque sample the transmittance is 1e-10 of what came before: w_k = T_k there, so every later weight is <= 1e-10 w_k,
        # and it is the reference's 1e-10 (not 0): the weights behind agree with fp64 RELATIVELY
        for r in range(c.R):
            k = int(torch.nonzero(c.opaque[r])[0])
            behind = d['w'][r, k + 1:].double()
            assert bool((behind <= 1.000001e-10 * float(d['w'][r, k])).all()), (label, r)
            rb = ref['w'][r, k + 1:]
            assert bool(((behind - rb).abs() <= 1e-4 * rb).all()), (label, r, behind, rb)
    if c.cls == 'zero_neg' and mode == 'softplus':
        neg = (c.sigma < 0) & (c.sigma > -20) & c.valid
        neg[:, -1] = False                                # (the last sample's 1e10 delta saturates it: exp(-s delta) = 0 and so is its gradient)
        assert bool(neg.any()) and bool((d['d_sigma'][neg] != 0).all()) and bool((out['c_sigma'][neg] != 0).all()), (label, 'softplus: no gradient at a negative sigma')


def check_capacity(R_over=None):
    """sherf_composite_compact_cap at its boundary.  Three consecutive rays (after two ordinary ones): one ends exactly at tok_cap and is rendered; an
    empty one has base == tok_cap and is rendered empty; one has base < tok_cap < base + cnt: NaN rgb / depth / acc and exactly bit 1 of counters[3].
    sample_out / cs_idx have exactly tok_cap rows, NaN / sentinel rows behind: a read behind the end would poison a rendered ray.
    R_over (the device): R_over rays, every one over capacity -- the flag is 2, not a sum."""
    S = 5
    if R_over is None:
        b = Rays('capacity', 'counts', S, 41)
        for v in (range(S), [1, 3], [0, 1, 2, 4], [], [0, 2, 3]):
            b.add(v, mix=False, empty=() if len(v) else MODES)
        c = b.done()
        tok_cap = int(c.base[2] + c.cnt[2])
        c.base[4] = tok_cap - 1                           # (the sampler's prefix sums would put it at tok_cap: by hand, so that it straddles the end)
        lost = torch.tensor([False, False, False, False, True])
        assert int(c.base[3]) == tok_cap and int(c.cnt[3]) == 0 and int(c.base[4]) < tok_cap < int(c.base[4] + c.cnt[4])
    else:
        b = Rays(f'capacity_R{R_over}', 'counts', S, 42)
        for r in range(R_over):
            b.add(range(S), mix=False)
        c = b.done()
        tok_cap = 3
        c.base += 1                                       # every ray: base < tok_cap < base + cnt, or beyond
        lost = torch.ones(R_over, dtype=torch.bool)
        assert bool(((c.base.long() + c.cnt.long()) > tok_cap).all()) and int(c.base[0]) < tok_cap
    for mode in MODES:
        for wb in (0, 1):
            for flag in (0, 1):                           # bit 0 (the MLP kernel's non-finite flag) is somebody else's and stays
                for batch1 in (False, True):
                    i = compact_inputs(c, tok_cap=tok_cap, flag=flag)
                    o = run_compact_forward(c, i, mode, wb, batch1=batch1)
                    assert o['counters'][:3].tolist() == i.counters0[:3].tolist() and int(o['counters'][3]) == (flag | 2), (mode, wb, flag, o['counters'][:4])
                    assert bool((o['counters'][4:] == SENT).all())
                    for k in ('rgb', 'depth', 'acc'):
                        assert bool(torch.isnan(o[k][lost]).all()) and bool(torch.isfinite(o[k][~lost]).all()), (mode, wb, k, o[k])
                    if R_over is None:
                        full = run_compact_forward(c, compact_inputs(c), mode, wb)          # the same rays with room for all of them
                        assert int(full['counters'][3]) == 0
                        for k in ('rgb', 'depth', 'acc'):
                            assert torch.equal(_bits(o[k][~lost]), _bits(full[k][~lost])), (mode, wb, k)
                        assert float(o['acc'][3]) == 0 and float(o['acc'][2]) > 0.5
    if R_over is None:                                    # everything fits exactly: no flag
        c.base[4] = tok_cap
        o = run_compact_forward(c, compact_inputs(c, flag=1), 'relu', 0)
        assert int(o['counters'][3]) == 1 and bool(torch.isfinite(o['rgb']).all())


def check_refusals():
    """Unknown mode bits, R <= 0, S = 0, tok_cap <= 0, a null output or input pointer, and S = 1 on the compact entry points (the dense ones take it:
    check_case('dense_S1')): SHERF_EINVAL before any launch -- every output keeps its sentinel."""
    L, P = _lib.lib(), _lib.ptr
    c = case('counts_S5')
    R, S = c.R, c.S
    i = compact_inputs(c)
    f32 = torch.float32
    rgb, dep, acc, w = _full((R + GUARD, 3), FSENT, f32), _full(R + GUARD, FSENT, f32), _full(R + GUARD, FSENT, f32), _full((R + GUARD, S), FSENT, f32)
    d_so, dc, ds = _full((c.nv + GUARD, 4), FSENT, f32), _full((R + GUARD, S, 3), FSENT, f32), _full((R + GUARD, S), FSENT, f32)
    col, sig, t, dmm = (G.dev_tensor(x.contiguous()) for x in (c.colors, c.sigma, c.t, torch.tensor([c.lo, c.hi])))
    g = {k: G.dev_tensor(v.contiguous()) for k, v in c.g.items()}
    st = _lib.stream()
    ins = (P(i.base), P(i.cnt), P(i.idx), P(i.so), P(i.rd), P(i.near), P(i.far))
    for kw in (dict(bits=4), dict(bits=-1), dict(R=0), dict(R=-5), dict(S=0), dict(tok_cap=0), dict(tok_cap=-1), dict(null='out'), dict(null='in'), dict(S=1)):
        r, s, bits, cap = kw.get('R', R), kw.get('S', S), kw.get('bits', 3), kw.get('tok_cap', i.tok_cap)
        n = (lambda x: None) if kw.get('null') == 'out' else (lambda x: x)
        m = (lambda x: None) if kw.get('null') == 'in' else (lambda x: x)
        ins = (P(i.base), P(i.cnt), P(i.idx), m(P(i.so)), P(i.rd), P(i.near), P(i.far))
        assert L.sherf_composite_compact_cap(P(i.counters), *ins, r, s, bits, cap, n(P(rgb)), P(dep), P(acc), st) == -1, kw
        assert b'bad argument' in L.sherf_last_error()
        if 'tok_cap' not in kw:
            assert L.sherf_composite_compact(P(i.counters), *ins, r, s, bits, n(P(rgb)), P(dep), P(acc), st) == -1, kw
            assert L.sherf_composite_compact_bwd(*ins, r, s, bits, P(g['rgb']), P(g['acc']), n(P(d_so)), st) == -1, kw
        if 'tok_cap' not in kw and kw.get('S') != 1:
            assert L.sherf_composite_dense(P(col), m(P(sig)), P(t), P(i.rd), r, s, bits, P(dmm), n(P(rgb)), P(dep), P(w), st) == -1, kw
            assert L.sherf_composite_dense_bwd(P(col), m(P(sig)), P(t), P(i.rd), r, s, bits, P(dmm), P(g['rgb']), P(g['depth']), P(g['w']), n(P(dc)), P(ds), st) == -1, kw
    _sync()
    for x in (rgb, dep, acc, w, d_so, dc, ds):
        assert bool((G.plain(x) == FSENT).all()), 'a refused call wrote something'
    assert torch.equal(G.plain(i.counters)[:4], i.counters0) and bool((G.plain(i.counters)[4:] == SENT).all())


def check_backward_refuses_an_overflowed_frame():
    """A no-grad forward whose token workspace was too small leaves NaN rays and bit 1 of counters[3]; sample_out then has fewer rows than the frame has
    valid samples, and sherf_composite_compact_bwd would read behind it.  composite_backward / render_backward refuse BEFORE any launch, and say what to
    re-size from."""
    from sherf_amd import backward
    G.hip_modules.cache_clear()
    rend, dec = G.hip_modules()
    mp = pytest.MonkeyPatch()
    mp.setattr(rend, 'TOKEN_GRANULE', 16, raising=False)
    launched = []
    real_call = _lib.call
    mp.setattr(_lib, 'call', lambda name, *a: (launched.append(name), real_call(name, *a))[1])
    real_call_bwd = _lib.call_bwd
    mp.setattr(_lib, 'call_bwd', lambda name, *a: (launched.append(name), real_call_bwd(name, *a))[1])
    try:
        worst = G.hip_render('tiny', options=dict(token_capacity='worst'))
        nv = int(worst['last']['ws']['counters'][0])
        last = worst['last']
        R = last['R']
        d_rgb, d_acc = G.dev_tensor(torch.ones(1, R, 3)), G.dev_tensor(torch.ones(1, R, 1))
        b = last['bwd']
        args = (b['ray_d'], b['near'], b['far'], b['white_back'], b.get('clamp_mode', 'relu'))
        ok = backward.composite_backward(rend, d_rgb, d_acc, *args)                # a frame that fitted: the backward runs
        assert ok.shape == (nv, 4) and bool(torch.isfinite(G.plain(ok)).all())
        small = G.hip_render('tiny', options=dict(token_capacity=nv // 2))
        last = small['last']
        assert last['cap'] < nv and int(last['ws']['counters'][3]) & 2 and last['ws']['sample_out'].shape[0] == last['cap']
        b = last['bwd']
        args = (b['ray_d'], b['near'], b['far'], b['white_back'], b.get('clamp_mode', 'relu'))
        del launched[:]
        with pytest.raises(RuntimeError, match=rf'overflowed its token workspace.*counters\[0\] = {nv}\b'):
            backward.composite_backward(rend, d_rgb, d_acc, *args)
        with pytest.raises(RuntimeError, match=rf'overflowed its token workspace.*counters\[0\] = {nv}\b'):
            backward.render_backward(rend, dec, d_rgb, d_acc)
        assert not launched, launched
    finally:
        mp.undo()
        G.hip_modules.cache_clear()


def check_reads_stay_inside():
    """HOST BUILD ONLY (tests/composite_guard_child.py, a process of its own): sample_out and cs_idx end at an inaccessible page, so that a read of the row
    behind a ray's last -- which the batched loads would make without their clamp to cnt - 1, and whose value no result depends on -- ends the process."""
    from tests.test_hipcpu_gather_edges import guarded_copy
    assert G.CPU_SHIM
    S = 9
    tails = []
    for n in (1, 2, 3, 5, 6, 7, 9):                       # the last ray's count: every remainder of the batch of four
        b = Rays(f'tail{n}', 'counts', S, 50 + n)
        b.add(range(S)); b.add([]); b.add(range(S - n, S))
        tails.append(b.done())
    for c in tails + [case('counts_S65'), case('rays_R257')]:
        i = compact_inputs(c)
        i.idx = guarded_copy(c.idx, 'end')
        i.so = guarded_copy(c.so.view(torch.int32), 'end').view(torch.float32).view(-1, 4)
        assert bool((i.so == c.so).all())
        for mode in MODES:
            full = run_compact_forward(c, compact_inputs(c), mode, 0)
            for batch1 in (False, True):
                o = run_compact_forward(c, i, mode, 0, batch1=batch1)
                assert all(torch.equal(_bits(o[k]), _bits(full[k])) for k in ('rgb', 'depth', 'acc'))
            b = run_compact_backward(c, i, mode, 0)
            assert bool(torch.isfinite(b['rows']).all())


# ---- the host build -------------------------------------------------------------------------------------------------------------------------------------------
def test_transcription_reproduces_the_reference_golden():
    check_transcription_against_golden()


@pytest.mark.parametrize('name', CASE_NAMES)
def test_rays(cpu_product, name):
    check_case(name)


def test_capacity_boundary(cpu_product):
    check_capacity()


def test_refusals(cpu_product):
    check_refusals()


def test_backward_refuses_an_overflowed_frame(cpu_product):
    check_backward_refuses_an_overflowed_frame()


def test_reads_stay_inside_the_compact_arrays():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, '-m', 'tests.composite_guard_child'], cwd=G.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0 and b'reads stayed inside' in r.stdout, (r.returncode, r.stdout.decode()[-2000:])


if __name__ == '__main__':                               # the table of FP32_REF_ERR
    for cls, row in fp32_reference_errors().items():
        print(f"    {cls!r}: dict(" + ', '.join(f'{q}={v:.2e}' for q, v in row.items()) + '),')
