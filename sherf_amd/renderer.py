"""MI355X-native `ImportanceRenderer`: drop-in for
/root/reference/sherf/training/volumetric_rendering/renderer.py:260-398 (same constructor flags, same
`forward` signature and return values, same parameter / buffer names), executing the whole hot loop with the
HIP kernels of sherf_amd/csrc through the C ABI in include/sherf_hip.h.

There is deliberately NO torch fallback: without the built library or off-GPU the forward raises.
Host-side torch ops are limited to plumbing: per-frame table re-layout + the "plain library GEMMs" that fold
the linear layers into the gather tables, and the tiny BatchNorm running-stat updates.
"""
import ctypes as _ct
import os
import pickle

import numpy as np
import torch
import torch.nn as nn

from . import _lib, mlp_pack, osg_pack
from .ray_marcher import MipRayMarcher2
from .voxel import SparseConvNet, SparseConvTensor, pack_conv_weights  # noqa: F401

# `prec` argument of sherf_nerf_mlp (include/sherf_hip.h): 'f16x3' = split fp16 operands, three MFMAs per product (fp32-grade);
# 'f16' = one fp16 product (11 bits); 'bf16' = one bf16 product (north_star's nominal precision, 8 bits).  `mlp_precision='auto'`
# (the default) is not a kernel mode: per set of weights it keeps the cheapest mode that reproduces f16x3 within a quarter of the
# 1e-3 tolerance on a whole frame of the weights' own samples (ImportanceRenderer._calibrate) -- 'f16' on networks of the reference's
# initialisation scale, 'f16x3' on the adversarial seeded test weights.
MLP_PRECISIONS = mlp_pack.PRECISIONS

V = 6890
NEAR_SUBCELLS = 524288        # SHERF_NEAR_SUBCELLS (include/sherf_hip.h)


def compute_normal(vertices, faces):
    """renderer.py:50-63. The reference's `norm[:, faces[:, c]] += n` is an index ASSIGNMENT: of the faces that list a
    vertex in column c exactly one contributes (the last on CPU, unspecified on CUDA). We take the highest face index,
    deterministically. vertices [B,V,3], faces [F,3]."""
    tris = vertices[:, faces]
    n = torch.cross(tris[:, :, 1] - tris[:, :, 0], tris[:, :, 2] - tris[:, :, 0], dim=-1)
    n = n / torch.sqrt((n ** 2).sum(-1, keepdim=True)).clamp_min(1e-8)
    norm = torch.zeros_like(vertices)
    nf = faces.shape[0]
    ar = torch.arange(nf, device=faces.device)
    for c in range(3):
        last = torch.full((vertices.shape[1],), -1, dtype=torch.long, device=faces.device).scatter_reduce_(0, faces[:, c], ar, reduce='amax')
        has = last >= 0
        norm[:, has] = norm[:, has] + n[:, last[has]]
    return norm / torch.sqrt((norm ** 2).sum(-1, keepdim=True)).clamp_min(1e-8)


# ---------------------------------------------------------------------------------------------------
# parameter containers with the reference's module tree (renderer.py:875-993)
# ---------------------------------------------------------------------------------------------------
class PositionalEncoding(nn.Module):
    """renderer.py:875-916 (buffers `_freqs`, `_phases` are part of the checkpoint contract)."""

    def __init__(self, num_freqs=6, d_in=3, freq_factor=None, include_input=True):      # (freq_factor: unused there as well, :884)
        super().__init__()
        self.num_freqs, self.d_in, self.include_input = num_freqs, d_in, include_input
        self.freqs = 2.0 ** torch.linspace(0.0, num_freqs - 1, steps=num_freqs)
        self.d_out = num_freqs * 2 * d_in + (d_in if include_input else 0)
        self.register_buffer('_freqs', torch.repeat_interleave(self.freqs, 2).view(1, -1, 1))
        ph = torch.zeros(2 * num_freqs)
        ph[1::2] = np.pi * 0.5
        self.register_buffer('_phases', ph.view(1, -1, 1))

    def forward(self, x):
        e = torch.sin(torch.addcmul(self._phases, x.unsqueeze(1).repeat(1, self.num_freqs * 2, 1), self._freqs))
        e = e.view(x.shape[0], self.num_freqs * 2 * self.d_in)
        return torch.cat((x, e), dim=-1) if self.include_input else e


class _Fn(nn.Module):           # Residual / PreNorm wrappers only contribute the `.fn` level of the key names
    def __init__(self, fn, norm_dim=None):
        super().__init__()
        if norm_dim is not None:
            self.norm = nn.LayerNorm(norm_dim)
        self.fn = fn


class _Attention(nn.Module):
    def __init__(self, dim, heads, dim_head):
        super().__init__()
        self.heads, self.scale = heads, dim_head ** -0.5
        self.to_qkv = nn.Linear(dim, heads * dim_head * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(heads * dim_head, dim), nn.Dropout(0.0))


class _FeedForward(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, hidden), nn.GELU(), nn.Dropout(0.0), nn.Linear(hidden, dim), nn.Dropout(0.0))


class Transformer(nn.Module):
    """renderer.py:980-993 with dim=32, depth=1, heads=3, dim_head=16, mlp_dim=32 (parameters only; the math runs
    inside sherf_nerf_mlp)."""

    def __init__(self, dim=32, depth=1, heads=3, dim_head=16, mlp_dim=32):
        super().__init__()
        assert (dim, depth, heads, dim_head, mlp_dim) == (32, 1, 3, 16, 32), 'fused kernel is specialised to the reference shape'
        self.layers = nn.ModuleList([nn.ModuleList([_Fn(_Fn(_Attention(dim, heads, dim_head), dim)),
                                                    _Fn(_Fn(_FeedForward(dim, mlp_dim), dim))])])


# ---------------------------------------------------------------------------------------------------
# SMPL asset (renderer.py:34-38, 65-74, 283-284)
# ---------------------------------------------------------------------------------------------------
def read_pickle(pkl_path):
    with open(pkl_path, 'rb') as f:
        u = pickle._Unpickler(f)
        u.encoding = 'latin1'
        return u.load()


def SMPL_to_tensor(params, device):
    """Same keys/dtypes as renderer.py:65-74, plus the derived constants the HIP kernels consume."""
    out = {}
    for k in ('v_template', 'shapedirs', 'weights', 'posedirs'):
        out[k] = torch.tensor(np.asarray(params[k]).astype(float), dtype=torch.float32, device=device)
    J = params['J_regressor']
    J = J.toarray() if hasattr(J, 'toarray') else np.asarray(J)
    out['J_regressor'] = torch.tensor(J.astype(float), dtype=torch.float32, device=device)
    out['kintree_table'] = torch.tensor(np.asarray(params['kintree_table']).astype(float), dtype=torch.long, device=device)
    out['f'] = torch.tensor(np.asarray(params['f']).astype(float), dtype=torch.long, device=device)
    # constants of the asset: J = J_regressor @ (v_template + shapedirs . beta) is linear in beta
    out['J_template'] = (out['J_regressor'] @ out['v_template']).contiguous()
    out['J_shapedirs'] = torch.einsum('jv,vcb->jcb', out['J_regressor'], out['shapedirs']).contiguous()
    par = out['kintree_table'][0].clone()
    par[0] = 0
    out['parents_i32'] = par.to(torch.int32).contiguous()
    out['posedirs_flat'] = out['posedirs'].reshape(V * 3, 207).contiguous()
    out['weights'] = out['weights'].contiguous()
    out['shapedirs'] = out['shapedirs'].contiguous()
    # for sherf_vertex_features (csrc/glue.hip): faces as int32 and, per face column, the highest face index listing each vertex
    f = np.asarray(params['f']).astype(np.int64)
    last = np.full((3, out['v_template'].shape[0]), -1, np.int32)
    for c in range(3):
        np.maximum.at(last[c], f[:, c], np.arange(f.shape[0], dtype=np.int32))
    out['f_i32'] = torch.tensor(f.astype(np.int32), dtype=torch.int32, device=device).contiguous()
    out['last_face_i32'] = torch.tensor(last, dtype=torch.int32, device=device).contiguous()
    return out


# ---------------------------------------------------------------------------------------------------
# host-side bookkeeping of a frame: the caches below are keyed on the parameters' (data_ptr, version), looked
# at EVERY frame -- through plain walks of the modules' own dicts (nn.Module.parameters() builds names, prefixes and a de-duplication set
# on the way: ~10x the cost), once per frame (`state_key` is memoised for the duration of a forward)
# ---------------------------------------------------------------------------------------------------
def fast_params(module, out=None, buffers=False):
    """Every parameter (buffers=True: and buffer) tensor below `module`, in registration order; shared tensors may repeat."""
    out = [] if out is None else out
    for p in module._parameters.values():
        if p is not None:
            out.append(p)
    if buffers:
        for b in module._buffers.values():
            if b is not None:
                out.append(b)
    for c in module._modules.values():
        if c is not None:
            fast_params(c, out, buffers)
    return out


def state_key(tensors):
    return tuple([(t.data_ptr(), t._version) for t in tensors])


# ---------------------------------------------------------------------------------------------------
# per-device workspace (sized for 288 GB of HBM: worst-case capacity, never reallocated per frame)
# ---------------------------------------------------------------------------------------------------
class _Workspace:
    def __init__(self):
        self.key = None
        self.t = {}
        self.vox = None
        self.bn = {}
        self.desc = None
        self.stacked = None
        self.tok_cap = 0
        # what the folded tables (planes_f / feat_f / img4) and the plan's voxel levels currently hold (rendering option `reuse_observation`):
        # the key of the last frame that encoded into them, the `levels` array that frame's native call filled in, and the keyed tensors
        # (kept referenced: a freed address cannot come back and compare equal)
        self.obs_key = None
        self.obs_levels = None
        self.obs_refs = None

    def frame(self, R, S, cap, dev):
        key = (R, S, cap, str(dev))
        if self.key == key:
            return self.t
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        nch = (S + 63) // 64
        t = dict(
            # counters: [0..3] the frame's (valid samples, depth min, depth max, flags); [4..6] `sticky` (sherf_frame.sticky: max count / OR of the flags / frames folded in)
            counters=torch.zeros(8, **i32), ray_base=torch.zeros(R, **i32), ray_cnt=torch.zeros(R, **i32),
            cs_idx=torch.zeros(cap, **i32), cs_vid=torch.zeros(cap, **i32),
            cs_xs=torch.zeros(cap, 4, **f32), dense_vid=torch.zeros(R * S, **i32),
            ray_mask=torch.zeros(R * nch, dtype=torch.int64, device=dev), scan_ws=torch.zeros(R + R // 1024 + 2, **i32),
            A=torch.zeros(3, 24, 12, **f32), posefeat=torch.zeros(3, 207, **f32), PO=torch.zeros(3, V, 3, **f32),
            SO=torch.zeros(3, V, 3, **f32), T2C=torch.zeros(V, 12, **f32), C2S=torch.zeros(V, 12, **f32),
            grid_hdr=torch.zeros(2, 12, **f32), cell_start=torch.zeros(2, 64 * 64 * 64 + 1, **i32),
            cell_pts=torch.zeros(2, V, 4, **f32), cell_scratch=torch.zeros(2 * 5 * V, **i32),
            near_mask=torch.zeros(32768, **i32),
            # sherf_build_near_lists: (start, count) per sub-cell of the near mask + the cursor; u16 vertex lists (worst case, never grown)
            near_hdr=torch.zeros(2 * NEAR_SUBCELLS + 2, **i32),
            near_list=torch.zeros(125 * V + 3 * NEAR_SUBCELLS, dtype=torch.int16, device=dev),
            # the candidate search by sub-cell (SHERF_CELL_WS_INTS): per-sub-cell counts (zero here, left zero by every frame) and offsets, the work items
            cell_ws=torch.zeros(4 * NEAR_SUBCELLS + 6 + 2 * (R * S // 64), **i32),
        )
        self.key, self.t = key, t
        self.desc = None
        self.tok_cap = 0
        self.obs_key = None                               # (a re-sized workspace never reuses what the old one held)
        self.tokens(min(cap, 256), dev)                   # (placeholders until the frame's own count is known: renderer._token_capacity)
        return t

    def tokens(self, tok_cap, dev):
        """The token-side buffers -- geom (32 B), tokens + extras (432 B), sample_out (16 B), cs_tvid (4 B per sample) -- for `tok_cap` compact
        samples: 484 of the workspace's ~510 bytes per sample, sized from the frame's OWN number of valid samples (a body fills 4-8 % of
        R * S) instead of the worst case."""
        if tok_cap == self.tok_cap:
            return
        f32 = dict(dtype=torch.float32, device=dev)
        tiles = (tok_cap + 31) // 32 + 8
        for k in ('geom', 'tokens', 'extras', 'sample_out', 'cs_tvid', 'zfrag', 'pefrag'):
            self.t.pop(k, None)                           # (free first: the new set may not fit beside the old one)
        self.t.update(geom=torch.zeros(tok_cap, 8, **f32), tokens=torch.zeros(tiles * 3 * 8 * 32 * 4, **f32),
                      extras=torch.zeros(tiles * 12 * 32, **f32), sample_out=torch.zeros(tok_cap, 4, **f32),
                      cs_tvid=torch.zeros(tok_cap, dtype=torch.int32, device=dev))
        self.tok_cap = tok_cap
        if self.desc is not None:                         # the cached descriptor follows (its other fields stay as they are)
            fr = self.desc[2]
            for k in ('geom', 'tokens', 'extras', 'sample_out', 'cs_tvid'):
                setattr(fr, k, _lib.addr(self.t[k]))
            fr.pefrag = None

    def pefrag(self, dev):
        """The positional encodings as fp16 MFMA operand fragments (SHERF_FRAME_PE_FRAGS: written by the gather, read by the network kernel):
        7 KiB per 32-sample tile = 224 B per sample, allocated with the token-side buffers' capacity the first time a frame asks for it."""
        z = self.t.get('pefrag')
        words = ((self.tok_cap + 31) // 32 + 8) * 7 * 64 * 4
        if z is None or z.numel() != words or z.device != torch.device(dev):
            z = self.t['pefrag'] = torch.zeros(words, dtype=torch.int32, device=dev)
        return z

    def nbytes(self):
        seen, n = set(), 0
        for v in list(self.t.values()) + list(self.bn.values()):
            if torch.is_tensor(v) and v.untyped_storage().data_ptr() not in seen:
                seen.add(v.untyped_storage().data_ptr()); n += v.untyped_storage().nbytes()
        return n

    STATIC_FIELDS = ('A', 'posefeat', 'PO', 'SO', 'T2C', 'C2S', 'grid_hdr', 'cell_start', 'cell_pts', 'cell_scratch', 'near_mask',
                     'counters', 'ray_base', 'ray_cnt', 'cs_idx', 'cs_vid', 'cs_xs', 'dense_vid', 'ray_mask', 'scan_ws', 'geom',
                     'cs_tvid', 'tokens', 'extras', 'sample_out', 'cell_ws')

    def descriptor(self, smpl):
        """The `sherf_frame` of this workspace with every field that does not change from frame to frame filled in ONCE (workspace and
        SMPL-asset pointers, sizes); forward() only writes the per-frame inputs into it.  (The native call reads it synchronously.)"""
        d = self.desc
        if d is not None and d[0] is self.t and d[1] is smpl:
            return d[2]
        A = _lib.addr
        fr = _lib.Frame()
        for k in self.STATIC_FIELDS:
            setattr(fr, k, A(self.t[k]))
        fr.sticky = A(self.t['counters']) + 16
        fr.cell_ws_len = self.t['cell_ws'].numel()
        fr.J_template, fr.J_shapedirs, fr.parents = A(smpl['J_template']), A(smpl['J_shapedirs']), A(smpl['parents_i32'])
        fr.posedirs, fr.shapedirs, fr.weights = A(smpl['posedirs_flat']), A(smpl['shapedirs']), A(smpl['weights'])
        self.desc = (self.t, smpl, fr, dict(near_hdr=A(self.t['near_hdr']), near_list=A(self.t['near_list']), near_cap=self.t['near_list'].numel()))
        return fr

    def zfrag(self, cap, prec_name, dev):
        """Scratch of sherf_nerf_mlp_split: the fused tokens as B-operand fragments, 4 KiB (8 KiB: f16x3) per 32-sample tile."""
        words = ((cap + 31) // 32 + 8) * (2048 if prec_name == 'f16x3' else 1024)
        z = self.t.get('zfrag')
        if z is None or z.numel() < words or z.device != torch.device(dev):
            z = self.t['zfrag'] = torch.empty(words, dtype=torch.int32, device=dev)
        return z

    def voxel_levels(self, shapes, N, dev):
        key = (tuple(shapes), N, str(dev))
        if self.vox is not None and self.vox[0] == key:
            return self.vox[1]
        i32 = dict(dtype=torch.int32, device=dev)
        dims = []
        for li, (D, H, W) in enumerate(shapes):
            nvox = D * H * W
            dims.append((nvox, (nvox + 31) // 32, N if li == 0 else min(nvox, 8 * N)))
        # one contiguous region for everything that must be zero at the start of a frame -> a single memset
        n_acc = 16 * 8 * 2 * 96 * 2                                         # BatchNorm accumulators: 16 layers x [8][2][96] int64
        zsize = sum(d[1] for d in dims) + N + N * 32 * 2 + 2 + n_acc + 2
        zsize = (zsize + 3) // 4 * 4                                        # (whole 16-byte blocks: the runtime clears them with ONE fill kernel, a ragged tail costs a second one)
        zero_region = torch.zeros(zsize, **i32)
        L, off = [], 0
        for li, (nvox, nwords, cap) in enumerate(dims):
            lv = dict(bitmap=zero_region[off:off + nwords], prefix=torch.zeros(nwords, **i32), keys=torch.zeros(cap, **i32),
                      n_rows=torch.zeros(1, **i32), chunk_ws=torch.zeros(nwords // 1024 + 2, **i32), wp=torch.zeros(nwords, 2, **i32),
                      nwords=nwords, cap=cap)
            off += nwords
            L.append(lv)
        L[0]['mult'] = zero_region[off:off + N]; off += N
        off += off % 2                                                     # 8-byte alignment of the fixed-point accumulators
        L[0]['acc_fix'] = zero_region[off:off + N * 64].view(torch.int64)
        off += N * 64
        L[0]['bn_acc'] = zero_region[off:off + n_acc].view(torch.int64)
        L[0]['g0'] = torch.zeros(N, 32, device=dev)
        L[0]['n_total'] = torch.full((1,), N, **i32)
        self.vox = (key, (L, zero_region))
        return self.vox[1]

    def _cached(self, kind, idx, shape, dev, dtype=torch.float32):
        k = (kind, idx, tuple(shape), str(dev))
        if k not in self.bn:
            self.bn[k] = torch.zeros(*shape, device=dev, dtype=dtype)
        return self.bn[k]

    def bn_stats(self, idx, C, dev):
        return self._cached('stats', idx, (2, C), dev)

    def bn_param(self, idx, C, dev):
        return self._cached('bnp', idx, (3, C), dev)

    def layer_out(self, idx, cap, C, dev):
        return self._cached('out', idx, (cap, C), dev)

    def fold_out(self, idx, cap, dev):
        return self._cached('fold', idx, (cap, 96), dev)

    def table(self, kind, shape, dev):
        return self._cached(kind, 0, shape, dev)


_SIDE_STREAMS = {}           # (device, caller stream) -> [side, aux]


class ImportanceRenderer(nn.Module):
    # beside `enable_autograd` (set per instance, or for the class by sherf_amd.install()): a renderer built with use_NeRF_decoder=False records its
    # grad-enabled forwards for the HIP backward only when this is set too -- the OSG backward is staged
    enable_osg_autograd = False
    # default of rendering_options['reuse_observation']: frame N + 1 of a camera / pose sweep renders from the folded tables and voxel levels frame N left
    # in the workspace when every input they are a function of is unchanged (_observation_key); opt-in
    reuse_observation = False

    def __init__(self, use_1d_feature=True, use_2d_feature=True, use_3d_feature=True, use_trans=False, use_NeRF_decoder=False,
                 smpl=None, smpl_path=os.path.join('assets', 'SMPL_NEUTRAL.pkl'), mlp_precision='auto', table_precision='auto', encoder_precision='auto'):
        super().__init__()
        self.use_1d_feature, self.use_2d_feature, self.use_3d_feature = use_1d_feature, use_2d_feature, use_3d_feature
        self.use_trans, self.use_NeRF_decoder = use_trans, use_NeRF_decoder
        self.ray_marcher = MipRayMarcher2()
        self.encoder_3d = SparseConvNet(num_layers=4)
        self.conv1d_projection = nn.Conv1d(192, 96, 1)
        if use_1d_feature and use_2d_feature and use_3d_feature:
            self.conv1d_reprojection = nn.Conv1d(96, 32, 1)
        elif (use_1d_feature and use_2d_feature) or (use_1d_feature and use_3d_feature) or (use_3d_feature and use_2d_feature):
            self.conv1d_reprojection = nn.Conv1d(64, 32, 1)
        self.transformer = None if not use_trans else Transformer(32)
        self.rgb_enc = PositionalEncoding(num_freqs=5)
        self.pos_enc = PositionalEncoding(num_freqs=6)
        self.view_enc = PositionalEncoding(num_freqs=4)
        self.mlp_precision = mlp_precision
        self.table_precision = table_precision            # 'auto' | 'f32' | 'f16'      (see _resolve_config)
        self.encoder_precision = encoder_precision        # 'auto' | 'f16x3' | 'f16'
        self.gather_split = os.environ.get('SHERF_GATHER_SPLIT', '0') == '1'   # tri-plane/pixel taps before the encoder join
        # schedule variant of the voxel taps (sherf_hip.h): False = one branch per corner, True = unconditional loads (160 VGPRs),
        # '128' = unconditional loads compiled for 4 waves / SIMD
        self.gather_branchless = {'0': False, '1': True, '128': '128'}[os.environ.get('SHERF_GATHER_BRANCHLESS', '0')]
        # SHERF_FRAME_EXACT_GRIDS (sherf_hip.h): launch warp / gather / MLP for the frame's actual valid-sample count (one host wait per
        # frame, where the reference has its own) instead of the R*S capacity; same results
        self.exact_grids = os.environ.get('SHERF_EXACT_GRIDS', '0') == '1'
        # the per-sample network as two launches (sherf_nerf_mlp_split): opt-in, measured slower than the one-launch kernel (see _set_config)
        self.mlp_split = {'': None, '0': False, '1': True}[os.environ.get('SHERF_MLP_SPLIT', '')]
        # launch form of the per-sample network for the single-product precisions (round 5; all forms give the same bits): 'pipelined' =
        # sherf_nerf_mlp3 (the decoder's layer epilogues inside the next ring step's MFMA stream; the default: 2-3 % faster on the MI355X),
        # 'two_tiles' = sherf_nerf_mlp2 (two tiles per wave), 'one' = sherf_nerf_mlp.  Rendering option `mlp_form`, default from SHERF_MLP_FORM
        # 'auto' (round 6, the default): the three forms give the same bits and the kernel runs at the board's power cap, where their ranking turned out to be a
        # property of the BOARD (evidence run 1: two tiles 0.506 ms, pipelined 0.532; other boxes: pipelined ahead by 1-3 %) -- so the first frame of a
        # (device, precision) renders its frame again in each form (whole frames: behind the frame's low-power first phase the kernel runs ~15 % faster than back to back, and the
        # forms rank differently there; 36 frames, once per process and board) and the process keeps the fastest (_tune_mlp_form)
        self.mlp_form = os.environ.get('SHERF_MLP_FORM', 'auto')
        # gather + per-sample network in N contiguous parts of the tile list, part k's network on the side stream beside part k + 1's
        # gather on the main one (sherf_hip.h: sherf_nerf_mlp_part; the same bits -- only the launch schedule differs); 0 / 1 = whole
        self.mlp_parts = int(os.environ.get('SHERF_MLP_PARTS', '0'))
        # token-side workspace (geom / tokens / extras / sample_out: 480 B per compact sample): 'auto' = sized from the frame's own number
        # of valid samples (first frame: the sampler alone + one host wait; later frames: the counts of finished frames, read without a
        # wait, grow it ahead of need), 'worst' = R * S as in rounds 1-3 (8 GB at 512 x 512 x 64), or a number of samples
        self.token_capacity = os.environ.get('SHERF_TOKEN_CAPACITY', 'auto')
        self.main_after_layer = int(os.environ.get('SHERF_MAIN_AFTER_LAYER', '-1'))   # stream scheduling, see sherf_frame
        self.aux_stream = os.environ.get('SHERF_AUX_STREAM', '1') == '1'           # voxel level structure on a third stream
        self._smpl_src = smpl
        self._smpl_path = smpl_path
        # not parameters / buffers (the reference keeps the SMPL dict as a plain attribute too, renderer.py:284);
        # excluded from pickling so module snapshots stay loadable without the asset or the .so handle.
        self._smpl_dev = None
        self._ws = {}                 # (device, caller stream) -> _Workspace
        self._wcache = None
        self.last = None

    def __getstate__(self):
        s = self.__dict__.copy()
        for k in ('_smpl_dev', '_ws', '_wcache', 'last', '_flags', '_frame_memo', '_pack_flag_pending', '_qws', 'last_query'):
            s[k] = None
        s['_ws'] = None
        return s

    def __setstate__(self, s):
        self.__dict__.update(s)
        self._ws = {}

    def _workspace(self, dev, main=None):
        """The frame workspace of the CALLER'S STREAM: frames issued on one stream share it (they are ordered anyway); frames issued
        round-robin on several streams -- the way to overlap frame N+1's low-occupancy first phase (cell lists, sampling, the encoder's
        chain of small launches) with frame N's chip-filling gather and MLP -- get one each, so nothing of frame N is overwritten
        while it is still in flight.  (A set costs ~0.5 KB per sample of capacity: 8 GB at 512x512x64 -- sized for 288 GB of HBM.)"""
        sid = (main or torch.cuda.current_stream(dev)).cuda_stream
        if self._ws is None or not isinstance(self._ws, dict):
            self._ws = {}
        key = (str(dev), sid)
        w = self._ws.pop(key, None)
        if w is None:
            w = _Workspace()
            # streams come and go, workspaces are gigabytes: at most MAX_WORKSPACES stay (least recently used goes; its frames are
            # waited for first -- a caller that creates a fresh stream per frame pays that wait instead of leaking a workspace per stream)
            while len(self._ws) >= self.MAX_WORKSPACES:
                old_key = next(iter(self._ws))
                if dev.type == 'cuda' and torch.cuda.is_available():
                    torch.cuda.synchronize(dev)
                del self._ws[old_key]
        self._ws[key] = w                                    # (re-inserted: dict order = recency)
        return w

    MAX_WORKSPACES = 8

    def _side(self, dev, idx=0):
        # ONE pair of side streams per device for every renderer of the process: HIP multiplexes streams onto 4 hardware queues, and a
        # second renderer with streams of its own (five in all) had two of its three streams share a queue -- its encoder chain and
        # ray side ran one after the other (3.1 instead of 1.9 ms per frame, profiles/r02_cfg3_as_headline.txt).  Frames of different
        # renderers are serialised by the native driver anyway.
        key = (dev, torch.cuda.current_stream(dev).cuda_stream)      # one pair per caller stream (see _workspace)
        cur = _SIDE_STREAMS.pop(key, None)
        if cur is None:
            # the short serial chains get dispatch priority over the ray side's big kernels
            xp = int(os.environ.get('SHERF_EXPERIMENT_STREAMS', '0'))     # (timing experiments of tools/frame_ab.py: 1 swap the pair, 2 default priority, 4 skip two queues)
            cur = [torch.cuda.Stream(device=dev, priority=0 if xp & 2 else -1) for _ in range(4 if xp & 4 else 2)][-2:]
            if xp & 1:
                cur.reverse()
            while len(_SIDE_STREAMS) >= 4 * self.MAX_WORKSPACES:     # bounded like the workspaces (streams of callers long gone)
                old = _SIDE_STREAMS.pop(next(iter(_SIDE_STREAMS)))
                for st in old:
                    st.synchronize()
        _SIDE_STREAMS[key] = cur
        return cur[idx]

    # ---- SMPL --------------------------------------------------------------------------------
    @property
    def SMPL_NEUTRAL(self):
        return self._smpl(torch.device('cuda', torch.cuda.current_device()))

    def _smpl(self, device):
        if self._smpl_dev is None or self._smpl_dev['v_template'].device != device:
            src = self._smpl_src if self._smpl_src is not None else read_pickle(self._smpl_path)
            self._smpl_dev = SMPL_to_tensor(src, device)
        return self._smpl_dev

    # ---- the two helpers the reference's TriPlaneGenerator.synthesis calls on its renderer (triplane.py:113,132) ------------
    def projection(self, query_pts, R, T, K, face=None):
        """renderer.py:686-704: pixel coordinates of `query_pts` [bs,N,3] in every view of R [bs,views,3,3], T [bs,views,3,1],
        K [bs,views,3,3] -> xy [bs,views,N,2]; with `face` also the mask of vertices whose normal faces the (first) camera.
        Per-frame glue over the 6890 vertices (not the hot path): plain device tensor ops."""
        R, T, K, q = R.float(), T.float(), K.float(), query_pts.float()
        xyz = torch.einsum('bvij,bnj->bvni', R, q) + T[:, :, None, :, 0]                       # [bs,views,N,3]
        mask = None
        if face is not None:
            normal = compute_normal(q, face)                                                   # [bs,N,3]
            ncam = torch.einsum('bvij,bnj->bvni', R, normal)
            mask = ((ncam * xyz).sum(-1) < 0).squeeze(1)                                       # renderer.py:693-695
        h = torch.einsum('bvij,bvnj->bvni', K, xyz)
        xy = h[..., :2] / (h[..., 2:] + 1e-5)
        return (xy, mask) if face is not None else xy

    def t2c_table(self, params, t_params):
        """Per-vertex affine of coarse_deform_target2c (renderer.py:558-621; SURVEY appendix A.5: x_c = P[j] x_s + q[j]) for the
        pose / shape in `params` against the canonical `t_params`, built by the HIP SMPL kernels -> T2C [V,12] = (P row-major | q)."""
        dev = params['poses'].device
        smpl = self._smpl(dev)
        f32 = lambda t: t.detach().float().contiguous()
        poses = torch.stack([f32(params['poses']).view(72), f32(t_params['poses']).view(72)])
        shapes = torch.stack([f32(params['shapes']).view(10), f32(t_params['shapes']).view(10)])
        A = torch.zeros(2, 24, 12, device=dev); pf = torch.zeros(2, 207, device=dev)
        PO = torch.zeros(2, V, 3, device=dev); SO = torch.zeros(2, V, 3, device=dev); T2C = torch.zeros(V, 12, device=dev)
        P, st = _lib.ptr, _lib.stream()
        _lib.call('sherf_smpl_bones', P(poses), P(shapes), 2, P(smpl['J_template']), P(smpl['J_shapedirs']), P(smpl['parents_i32']),
                  P(A), P(pf), st)
        _lib.call('sherf_smpl_offsets', P(smpl['posedirs_flat']), P(smpl['shapedirs']), P(pf), P(shapes), 2, P(PO), P(SO), st)
        _lib.call('sherf_smpl_t2c_table', P(smpl['weights']), P(A[0]), P(A[1]), P(PO[0]), P(SO[0]), P(PO[1]), P(T2C), st)
        return T2C

    def coarse_deform_target2c(self, params, vertices, t_params, query_pts, query_viewdirs=None):
        """renderer.py:558-621 for callers outside the frame (triplane.py:132 passes the posed vertices themselves): nearest posed
        vertex of every query point (exact, lowest index on ties), then that vertex's target->canonical affine from the HIP SMPL
        kernels.  Inside `forward` the same table is applied by the fused warp kernel; this method is per-frame glue."""
        if query_pts.shape[0] != 1:
            raise RuntimeError('per-GPU batch must be 1, as in the reference (renderer.py:567)')
        f32 = lambda t: t.detach().float().contiguous()
        T2C = self.t2c_table(params, t_params)
        xs = torch.matmul(f32(vertices).view(V, 3) - f32(params['Th']).view(1, 3), f32(params['R']).view(3, 3))
        q = f32(query_pts).view(-1, 3)
        if q.shape[0] == V and torch.equal(q, xs):
            vid = torch.arange(V, device=q.device)                        # every vertex is its own nearest vertex
        else:
            vid = torch.cat([(((c[:, None, 0] - xs[None, :, 0]) ** 2 + (c[:, None, 1] - xs[None, :, 1]) ** 2)
                              + (c[:, None, 2] - xs[None, :, 2]) ** 2).argmin(1) for c in q.split(8192)])
        Pm, t = T2C[vid, :9].view(-1, 3, 3), T2C[vid, 9:]
        can = (torch.einsum('nij,nj->ni', Pm, q) + t).view(1, -1, 3)
        if query_viewdirs is not None:
            return can, torch.einsum('nij,nj->ni', Pm, f32(query_viewdirs).view(-1, 3)).view(1, -1, 3)
        return can

    def check_finite(self):
        """True unless the MLP kernel of the LAST frame produced a non-finite sigma / rgb (its fp16 operand modes overflow beyond
        65504: csrc/mlp.hip sets counters[3]).  Synchronises with the frame; call it when validating a checkpoint, not per frame."""
        return self.last is None or (int(self.last['ws']['counters'][3]) & 3) == 0      # (bit 1: the token-side workspace overflowed)

    # ---- `auto` stays honest after its calibration --------------------------------------------------
    AUTO_RECHECK_EVERY = int(os.environ.get('SHERF_AUTO_RECHECK', '256'))     # frames between re-calibrations of a kept choice (3 extra frames each)

    def _auto_state_key(self):
        """What the calibrated choice depends on besides the MLP's own parameters (those key the weight cache): the sparse encoder's
        parameters AND buffers (BatchNorm running statistics): they set the magnitude of the fp16 tables' error."""
        # (train-mode BatchNorm normalises with batch statistics and MOVES the running ones every frame: parameters only there)
        enc = self.encoder_3d
        pk = enc.__dict__.get('_key_memo') or state_key(fast_params(enc))
        # (and the density activation the candidates were scored under: _calibrate; a choice is kept per clamp mode, _auto_for_mode)
        mode = (self.__dict__.get('_clamp_mode', 'relu'),)
        if enc.training:
            return (True,) + mode + pk
        return (False,) + mode + pk + state_key([b for m in enc.modules() for b in m._buffers.values() if b is not None])

    _AUTO_STATE = ('auto', 'auto_key', 'auto_frames', 'auto_tripped')

    def _auto_for_mode(self, wc):
        """The calibrated choice belongs to the clamp mode it was measured under: when the frame's mode differs from the one the weight cache
        holds a choice for, that choice is put aside and the other mode's (or none) taken up -- a renderer used under both modes calibrates each once."""
        mode, held = self.__dict__.get('_clamp_mode', 'relu'), wc.get('auto_mode', 'relu')
        if mode != held:
            per = wc.setdefault('auto_per_mode', {})
            per[held] = {k: wc.get(k) for k in self._AUTO_STATE}
            wc.update(per.get(mode) or dict.fromkeys(self._AUTO_STATE))
            wc['auto_mode'] = mode

    WATCH_RING = int(os.environ.get('SHERF_WATCH_RING', '4'))      # pinned slots of the read-back ring = frames the host may run ahead when every frame is read back
    WATCH_EVERY = int(os.environ.get('SHERF_WATCH_EVERY', '8'))     # frames between two read-backs of the counters (every frame's flags reach the sticky words on the device meanwhile)

    def _note_counters(self, st, c, ws=None):
        """c = a workspace's eight counter words read back: [0..3] the last frame's (count, ., ., flags), [4..6] what the frames before it left (sticky)."""
        flags, nv = c[3] | (c[5] if len(c) > 5 else 0), max(c[0], c[4] if len(c) > 4 else 0)
        if flags & 1:
            st['tripped'] += 1                             # an fp16 operand beyond 65504 in some frame since the last read-back
        if flags & 2:                                      # more valid samples than the token-side workspace held: NaN rays in that frame
            st['overflowed'] = st.get('overflowed', 0) + 1
        st['nv_seen'] = max(st.get('nv_seen', 0), nv)
        if ws is not None and len(c) > 5 and (c[5] or c[4]):
            ws['counters'][4:7].zero_()                    # (sticky words are the host's to clear; rare for the flags, cheap for the count: behind a read-back only)

    def _flag_watch(self, ws, dev):
        """The MLP kernel's non-finite flag (counters[3] bit 0: an fp16 operand beyond 65504) and the token-overflow flag of EVERY frame, without a host wait and --
        round 6 -- without a read-back behind every frame (the 32-byte copy + its event cost the caller's stream ~15 us per frame, tools/tail_probe.py): the frame
        driver folds each frame's counters into sticky words on the device (sherf_frame.sticky) when the next frame resets them, and the words are copied to pinned
        memory every WATCH_EVERY frames and read once their event has passed.  A trip drops the calibrated choice (the next frame re-calibrates, i.e. renders in the
        fp32-grade configuration) and is reported once."""
        st = self.__dict__.setdefault('_flags', dict(ring=[], tripped=0))
        seen = st.setdefault('watched', {})                # (poll_flags(wait=True) reads the newest frames' words of every workspace directly)
        seen[ws['counters'].data_ptr()] = ws['counters']
        while len(seen) > 16:
            seen.pop(next(iter(seen)))
        if dev.type != 'cuda' or getattr(ws['counters'], 'device', dev).type != 'cuda':      # host build of the tests: read directly
            self._note_counters(st, ws['counters'].tolist(), ws)
            return st
        ring = st['ring']
        for other in ring:                                 # anything already finished is read now
            if other['busy'] and other['ev'].query():
                other['busy'] = False
                self._note_counters(st, other['host'].tolist())
        since, key = st.setdefault('since', {}), ws['counters'].data_ptr()      # per workspace: frames issued round-robin on several streams each keep their own count
        # Frames issued round-robin on SEVERAL caller streams are read back every frame, as in rounds 4-5: waiting for the ring's oldest slot is what keeps the host at most four
        # frames ahead there, and without that throttle the streams' queues run deep and the frames overlap worse (four streams: 1.37 -> 1.54-1.64 ms per frame,
        # profiles/r06_ad_*); the read-back's own cost hides behind the other streams' frames in that mode.
        every = 1 if isinstance(self._ws, dict) and len(self._ws) > 1 else self.WATCH_EVERY
        since[key] = since.get(key, every - 1) + 1                          # (the first frame on a workspace is read back)
        if since[key] < every:
            return st
        since[key] = 0
        while len(since) > 16:
            since.pop(next(iter(since)))
        if len(ring) < self.WATCH_RING:
            ring.append(dict(host=torch.zeros(8, dtype=torch.int32).pin_memory(), ev=torch.cuda.Event(), busy=False))
            st['next'] = len(ring) - 1
        slot = ring[st.get('next', 0) % len(ring)]
        st['next'] = (st.get('next', 0) + 1) % self.WATCH_RING
        if slot['busy']:
            slot['ev'].synchronize()                       # (4 x WATCH_EVERY frames old: long done)
            self._note_counters(st, slot['host'].tolist())
        slot['host'].copy_(ws['counters'], non_blocking=True)
        ws['counters'][4:7].zero_()                        # the sticky words start over behind the copy (same stream: ordered)
        slot['ev'].record(torch.cuda.current_stream(dev))
        slot['busy'] = True
        return st

    def poll_flags(self, wait=False):
        """The watch's state (`tripped`, `overflowed`, `nv_seen`, ...) after reading every finished read-back; wait=True also waits for the frames still in flight and
        reads the newest frames' counters directly (one host wait)."""
        st = self.__dict__.setdefault('_flags', dict(ring=[], tripped=0))
        for slot in st['ring']:
            if slot['busy'] and (wait or slot['ev'].query()):
                slot['ev'].synchronize()
                slot['busy'] = False
                self._note_counters(st, slot['host'].tolist())
        if wait:
            for w in list((st.get('watched') or {}).values()):
                if w.device.type == 'cuda':
                    torch.cuda.synchronize(w.device)       # (frames of other caller streams included)
                self._note_counters(st, w.tolist(), dict(counters=w))
        return st

    TOKEN_HEADROOM = 1.5         # token-side capacity = this x the largest count seen, re-sized when a frame passes TOKEN_GROW_AT of it
    TOKEN_GROW_AT = 0.8

    TOKEN_GRANULE = 8192

    def _round_tokens(self, n, cap):
        g = self.TOKEN_GRANULE
        return int(min(cap, max(g, (int(n) + g - 1) // g * g)))

    def _token_capacity(self, opts, wsp, cap, dev, probe):
        """Samples the token-side buffers of `wsp` should hold for this frame (see `token_capacity` in __init__).  `probe()` runs the
        sampler alone and returns the frame's valid-sample count (one host wait): used when the workspace has never seen a frame."""
        want = opts.get('token_capacity', getattr(self, 'token_capacity', 'auto'))
        if want in ('worst', None) or (torch.is_grad_enabled() and getattr(self, 'enable_autograd', False)) or getattr(self, '_in_autograd', False):
            return cap                                     # (training: the backward sizes its own matrices from the count it reads anyway)
        if want != 'auto':
            return self._round_tokens(int(want), cap)
        st = self.__dict__.setdefault('_flags', dict(ring=[], tripped=0))
        seen = wsp.__dict__.setdefault('nv_sized_for', None)
        if seen is None:                                   # first frame on this workspace
            nv = probe()
            wsp.nv_sized_for = nv
            self.poll_flags(wait=True)                     # (the probe waited for the device anyway: counts still in the ring belong to the past)
            st['nv_seen'] = 0
            wsp.t['counters'][4:7].zero_()                 # (and so does what earlier frames left in the sticky words)
            return self._round_tokens(self.TOKEN_HEADROOM * nv, cap)
        nv = st.get('nv_seen', 0)
        if nv > self.TOKEN_GROW_AT * wsp.tok_cap and wsp.tok_cap < cap:
            wsp.nv_sized_for = nv
            st['token_regrowths'] = st.get('token_regrowths', 0) + 1
            return self._round_tokens(self.TOKEN_HEADROOM * nv, cap)
        return wsp.tok_cap

    def drain_pack_flag(self):
        """The weight-range flag word of the LAST training repack (read back one step late while training, _pack_stream): checked now.  Called when
        training stops -- eval() / train(False) -- so that the final step's out-of-range or non-finite weights do not go unreported."""
        pend = self.__dict__.pop('_pack_flag_pending', None)
        if pend is not None:
            pend[0].synchronize()
            mlp_pack.raise_for_flags(int(pend[1][0]), 0.0, pend[2])

    def train(self, mode=True):
        if not mode:
            self.drain_pack_flag()
        return super().train(mode)

    # ---- weights -----------------------------------------------------------------------------
    def _weights(self, decoder, device, precision=None):
        """Packed weights for the frame: the fold tables (precision independent) + the MLP fragment stream in `precision`.  Cached on
        the parameters' (data_ptr, version): an optimiser step or load_state_dict repacks, a second precision of the same weights
        only adds its stream."""
        precision = precision or self.mlp_precision
        prec = MLP_PRECISIONS[precision]
        memo = self.__dict__.get('_frame_memo')                # (set for the duration of a forward: one walk per frame, not one per caller)
        if memo is not None and memo[0] is decoder and memo[1] == device:
            key = memo[2]
        else:
            ps = []
            for m in (self.conv1d_projection, getattr(self, 'conv1d_reprojection', None), self.transformer, decoder):
                if m is not None:                       # (use_trans = False: no transformer)
                    fast_params(m, ps)
            key = state_key(ps) + (str(device),)
            if memo is not None:
                self.__dict__['_frame_memo'] = (decoder, device, key)
        wc = self._wcache
        if wc is None or wc['key'] != key:
            Wr, br = self._effective_reprojection()                                  # [32, 96], [32]
            Wp = self.conv1d_projection.weight.detach().float()[:, :, 0]            # [96, 192]
            bp = self.conv1d_projection.bias.detach().float()
            Wa, Wb, Wc = Wr[:, 0:32], Wr[:, 32:64], Wr[:, 64:96]
            cols = ((0, 32), (32, 96), (96, 192))
            fold = []
            for c0, c1 in cols:             # F_l [96, C_l]: rows 32s.. = W_c @ W_p[32s:32s+32, cols_l]
                F = torch.cat([Wc @ Wp[32 * s:32 * s + 32, c0:c1] for s in range(3)], 0)
                fold.append(pack_conv_weights(F.t().contiguous()[None]).to(device))   # [C_l, 96] as a 1-tap conv
            tok_bias = torch.cat([br + Wc @ bp[32 * s:32 * s + 32] for s in range(3)]).contiguous().to(device)
            wc = self._wcache = dict(key=key, Wa_t=Wa.t().contiguous().to(device), Wb_t=Wb.t().contiguous().to(device), fold=fold,
                                     tok_bias=tok_bias, streams={}, auto=None, flat=None)
        if not self.use_NeRF_decoder:
            # OSG path: ONE fp32 weight block whatever the tables' / encoder's precision (sherf_osg_decoder), cached like the NeRF streams
            if 'osg' not in wc['streams']:
                wc['streams']['osg'] = (self._pack_osg(decoder, device), None)
            prec = 'osg'
        elif prec not in wc['streams']:
            wc['streams'][prec] = self._pack_stream(decoder, device, prec, wc)
        out = dict(wc)
        out['stream'], out['wbias'] = wc['streams'][prec]
        return out

    @staticmethod
    def _osg_layers(decoder):
        """(net.0, net.2) of an OSGDecoder -- this package's or, duck-typed, the reference's own instance (triplane.py:242-251) -- else TypeError."""
        net = getattr(decoder, 'net', None)
        try:
            l0, l2 = net[0], net[2]
            ok = tuple(l0.weight.shape) == (64, 32) and tuple(l2.weight.shape) == (4, 64) and tuple(l0.bias.shape) == (64,) and tuple(l2.bias.shape) == (4,)
        except Exception:
            ok = False
        if not ok:
            raise TypeError(f'this renderer was built with use_NeRF_decoder=False and needs an OSGDecoder (net.0: 32 -> 64, net.2: 64 -> 4) as `decoder`, '
                            f'not {type(decoder).__name__}')
        return l0, l2

    def _check_decoder(self, decoder):
        """The `decoder` handed to forward must be of the kind the constructor's use_NeRF_decoder switch selects."""
        if not self.use_NeRF_decoder:
            self._osg_layers(decoder)
        elif not (hasattr(decoder, 'pts_linears') and hasattr(decoder, 'alpha_linear')):
            raise TypeError(f'this renderer was built with use_NeRF_decoder=True and needs a NeRFDecoder as `decoder`, not {type(decoder).__name__}')

    def _pack_osg(self, decoder, device):
        """The fp32 weight block of sherf_osg_decoder (include/sherf_hip.h), gathered ON THE DEVICE from the live parameters through osg_pack's index
        map: W_b of the EFFECTIVE reprojection matrix (switched-off feature branches: zero blocks), the head's two FullyConnectedLayers with their
        run-time gains folded in (weight_gain / bias_gain of the module where present: networks_stylegan2.py:96-131), the transformer if there is one."""
        l0, l2 = self._osg_layers(decoder)
        f = lambda t: t.detach().to(device=device, dtype=torch.float32).reshape(-1)
        Wr, _ = self._effective_reprojection()
        flat = [f(Wr[:, 32:64].contiguous())]
        for l in (l0, l2):
            flat += [f(l.weight) * float(getattr(l, 'weight_gain', 1.0)), f(l.bias) * float(getattr(l, 'bias_gain', 1.0))]
        if self.transformer is not None:
            named = dict(self.transformer.layers[0].named_parameters())
            flat += [f(named[n]) for n, _, _ in osg_pack.TRANS_PARAMS]
        flat = torch.cat(flat + [torch.zeros(1, device=device)])                   # (last element: the zero that absent slots read)
        src, n_flat = osg_pack.block_index(self.transformer is not None)
        if flat.numel() != n_flat + 1:
            raise RuntimeError('sherf_amd: parameter shapes do not match the OSG weight block')
        cache = self.__dict__.setdefault('_pack_index', {})
        ikey = ('osg', self.transformer is not None, str(device))
        idx = cache.get(ikey)
        if idx is None:
            idx = cache[ikey] = torch.from_numpy(np.where(src >= 0, src, n_flat)).to(device)
        block = flat[idx].contiguous()
        if not bool(torch.isfinite(block).all()):
            raise ValueError('non-finite values in the reprojection / transformer / OSGDecoder weights; the OSG weight block cannot be packed')
        return block

    def feature_branches(self):
        """(1d, 2d, 3d): which feature branches reach the fused tokens -- the constructor's switches read the way run_model's if / elif chain reads
        them (renderer.py:405-425): all three; any two; otherwise the tri-plane features alone, whatever the remaining switches say (the chain has no
        branch for a single 2-D or 3-D source: `sampled_features` stays the plane samples)."""
        a, b, c = bool(self.use_1d_feature), bool(self.use_2d_feature), bool(self.use_3d_feature)
        return (a, b, c) if a + b + c >= 2 else (True, False, False)

    def _effective_reprojection(self):
        """conv1d_reprojection as the [32, 96] matrix over [tri-plane | pixel-aligned | voxel] features + bias that the folded tables, the gather and
        the network's slot-2 completion are built on, for EVERY combination of use_1d/2d/3d_feature (round 6; renderer.py:266-269, 405-425): a
        two-branch renderer owns a Conv1d(64, 32) whose two 32-column blocks act on the two branches it has, in the order 1d, 2d, 3d -- the missing
        branch's block is zero (its taps then add exact zeros: same sums as not taking them); tri-plane features alone pass through unprojected
        (identity, no bias; there is no conv1d_reprojection module then)."""
        on = self.feature_branches()
        if sum(on) == 3:
            return self.conv1d_reprojection.weight.detach().float()[:, :, 0], self.conv1d_reprojection.bias.detach().float()
        dev = self.conv1d_projection.weight.device
        W = torch.zeros(32, 96, device=dev)
        if sum(on) == 1:
            W[:, 0:32] = torch.eye(32, device=dev)
            return W, torch.zeros(32, device=dev)
        Wr = self.conv1d_reprojection.weight.detach().float()[:, :, 0]
        k = 0
        for i in range(3):
            if on[i]:
                W[:, 32 * i:32 * i + 32] = Wr[:, 32 * k:32 * k + 32]
                k += 1
        return W, self.conv1d_reprojection.bias.detach().float()

    def _pack_stream(self, decoder, device, prec, wc):
        """The MLP's fragment stream + bias table for `prec`, packed ON THE DEVICE from the live parameters (sherf_mlp_pack_stream applying
        mlp_pack.stream_index's element map: bit-identical to the host packer mlp_pack.pack, tests/test_mlp_pack.py, at ~0.1 ms
        instead of ~45 ms -- a training step repacks after every optimiser update).  The fp16 range checks of the host packer
        (mlp_pack.check_f16_range) are made on the device and read back once per repack: same ValueError."""
        named = {'renderer.' + k: v for k, v in self.named_parameters() if not k.startswith('encoder_3d.')}
        named.update({'decoder.' + k: v for k, v in decoder.named_parameters()})
        if sum(self.feature_branches()) != 3:
            # fewer than three feature branches (round 6): the stream's slot-2 completion W_b . PE5(rgb) takes the EFFECTIVE [32, 96] matrix
            Wr, br = self._effective_reprojection()
            named['renderer.conv1d_reprojection.weight'], named['renderer.conv1d_reprojection.bias'] = Wr[:, :, None].to(device), br.to(device)
        if self.transformer is None:
            # use_trans = False (renderer.py:261, 427): the kernel walks past the transformer's chunks (SHERF_MLP_NO_TRANSFORMER); their slots of the
            # stream are packed from zeros so that the layout -- and every other chunk's place in it -- stays the one the kernel knows
            z = lambda *sh: torch.zeros(*sh, device=device)
            t = 'renderer.transformer.layers.0.'
            named.update({t + '0.fn.norm.weight': z(32), t + '0.fn.norm.bias': z(32), t + '0.fn.fn.to_qkv.weight': z(144, 32), t + '0.fn.fn.to_out.0.weight': z(32, 48),
                          t + '0.fn.fn.to_out.0.bias': z(32), t + '1.fn.norm.weight': z(32), t + '1.fn.norm.bias': z(32), t + '1.fn.fn.net.0.weight': z(32, 32),
                          t + '1.fn.fn.net.0.bias': z(32), t + '1.fn.fn.net.3.weight': z(32, 32), t + '1.fn.fn.net.3.bias': z(32)})
        names = mlp_pack.packed_names()
        if wc.get('flat') is None:
            wc['flat'] = torch.cat([named[n].detach().to(device=device, dtype=torch.float32).reshape(-1) for n in names])
        flat = wc['flat']
        ikey = (prec, str(device))
        cache = self.__dict__.setdefault('_pack_index', {})          # (plain attribute: not a parameter / buffer / submodule)
        idx = cache.get(ikey)
        if idx is None:
            src, bsrc, n_flat = mlp_pack.stream_index({n: tuple(named[n].shape) for n in names}, prec=prec)
            idx = cache[ikey] = (torch.from_numpy(src).to(device), torch.from_numpy(bsrc).to(device), n_flat)
        src, bsrc, n_flat = idx
        if flat.numel() != n_flat:
            raise RuntimeError('sherf_amd: parameter shapes changed under a cached stream index')
        stream = torch.empty(2 * src.numel(), dtype=torch.uint8, device=device)
        wbias = torch.empty(bsrc.numel(), dtype=torch.float32, device=device)
        flag = torch.empty(1, dtype=torch.int32, device=device)
        P = _lib.ptr
        _lib.call('sherf_mlp_pack_stream', P(flat), P(src), src.numel(), prec, P(stream), P(bsrc), bsrc.numel(), P(wbias), P(flag), _lib.stream())
        if getattr(self, '_in_autograd', False) and device.type == 'cuda' and flag.device.type == 'cuda':
            # Training: a repack follows every optimiser update, and reading its flag word back HERE made the host wait for the previous step's
            # kernels (19.5 ms of host time per step in bench_train.py, rounds 3-4).  The word goes to pinned memory behind the pack kernel
            # instead and is looked at by the NEXT repack, a whole step later, when it has long landed: the same ValueError, one step late
            # (weights move a little per step from a checked start; the kernel's own non-finite flag, check_finite(), stays armed meanwhile).
            pend = self.__dict__.get('_pack_flag_pending')
            if pend is not None:
                pend[0].synchronize()
                mlp_pack.raise_for_flags(int(pend[1][0]), 0.0, pend[2])
                ev, host = pend[0], pend[1]                        # (one pinned word and one event per renderer: the last pair has just been consumed)
            else:
                ev, host = torch.cuda.Event(), torch.empty(1, dtype=torch.int32).pin_memory()
            host.copy_(flag, non_blocking=True)
            ev.record()
            self.__dict__['_pack_flag_pending'] = (ev, host, prec, flag)
            return stream, wbias
        self.drain_pack_flag()                                     # (a repack outside training: the last training step's word is due now)
        checks = [flag.to(torch.float32)]
        if prec != 0 and not getattr(self, '_in_autograd', False):
            # a-priori bound of the activations (mlp_pack.check_f16_range): product of the layers' row norms.  Skipped while training
            # (weights move a little per step from a checked start; the kernel's own non-finite flag, check_finite(), stays armed)
            bound = torch.full((), 64.0, dtype=torch.float64, device=device)
            for lname in [f'decoder.pts_linears.{i}' for i in range(8)] + ['decoder.feature_linear', 'decoder.views_linear']:
                W, b = named[lname + '.weight'].detach().double(), named[lname + '.bias'].detach().double()
                bound = bound * W.abs().sum(1).max() + b.abs().max()
            checks.append(bound.clamp(max=1e38).to(torch.float32).reshape(1))
        vals = torch.cat(checks).tolist()
        mlp_pack.raise_for_flags(int(vals[0]), vals[1] if len(vals) > 1 else 0.0, prec)
        return stream, wbias

    # ---- precision configuration ----------------------------------------------------------------
    # A frame's configuration = (MLP operand precision, format of the folded tables the gather taps, operand precision of the sparse
    # convolutions).  'f16x3' / fp32 tables / 'f16x3' is the fp32-grade reference configuration.  mlp_precision='auto' measures the
    # cheaper ones, cheapest first, against it on a whole frame of the weights' own samples and keeps the first within AUTO_TOL.
    REFERENCE_CONFIG = ('f16x3', 'f32', 'f16x3')
    # cheapest first.  ('f16', 'f16', 'f16') -- single-product sparse convolutions too -- is a candidate again in round 4: round 3's "wrong
    # folded rows on the MI355X" was an MFMA that hipcc had predicated by EXEC without a skip branch (csrc/svox.hip: `wave`), fixed and
    # guarded by tests/test_isa_hazards.py; the calibration measures it on the frame like every other candidate
    AUTO_CANDIDATES = (('f16', 'f16', 'f16'), ('f16', 'f16', 'f16x3'), ('f16', 'f32', 'f16x3'))
    AUTO_TOL = 2.5e-4                   # a quarter of north_star's 1e-3 per-sample budget (true relative error, floors 1.0 / 0.1)

    def _resolve_config(self, opts, decoder, dev):
        """-> ((mlp, tables, encoder), calibrate?).  Explicit settings win (rendering_options, then the constructor's); 'auto' tables
        are fp16 exactly when the MLP runs on single products (its first MFMA rounds the tokens to 11 / 8 bits anyway); an 'auto'
        encoder stays f16x3 unless mlp_precision='auto' measured the single-product convolutions acceptable on the frame.  The autograd path stays fp32-grade throughout: weights
        change every step and the backward reads fp32 tables."""
        mlp = opts.get('mlp_precision') or self.mlp_precision
        tab = opts.get('table_precision') or getattr(self, 'table_precision', 'auto')
        enc = opts.get('encoder_precision') or getattr(self, 'encoder_precision', 'auto')
        training = getattr(self, '_in_autograd', False) or (torch.is_grad_enabled() and getattr(self, 'enable_autograd', False))
        if training:
            return (mlp if mlp != 'auto' else 'f16x3', 'f32', 'f16x3'), False
        if mlp == 'auto' and not self.use_NeRF_decoder:
            # OSG path: the head is fp32 whatever the setting; `mlp_precision` only selects the tables' / encoder's precision there, and 'auto' is
            # the fp32-grade configuration without a calibration frame
            return self.REFERENCE_CONFIG, False
        if mlp == 'auto':
            self._weights(decoder, dev, 'f16x3')
            wc = self._wcache
            self._auto_for_mode(wc)
            choice = wc['auto']
            if choice is not None and choice != self.REFERENCE_CONFIG:
                # a kept cheaper configuration is re-measured when anything it was measured under may have moved: the encoder's weights /
                # statistics, AUTO_RECHECK_EVERY frames (other poses, cameras, subjects under the same weights), a tripped non-finite flag
                st = self.__dict__.get('_flags') or {}
                why = ('encoder state changed' if wc.get('auto_key') != self._auto_state_key() else
                       'non-finite flag' if st.get('tripped', 0) > wc.get('auto_tripped', 0) else
                       'periodic' if wc.get('auto_frames', 0) >= self.AUTO_RECHECK_EVERY else None)
                if why:
                    wc['auto_recalibrations'] = wc.get('auto_recalibrations', []) + [why]
                    choice = wc['auto'] = None
            if choice is None:
                return self.REFERENCE_CONFIG, True
            wc['auto_frames'] = wc.get('auto_frames', 0) + 1
            mlp, t0, e0 = choice
            return (mlp, t0 if tab == 'auto' else tab, e0 if enc == 'auto' else enc), False
        tab = tab if tab != 'auto' else ('f16' if mlp in ('f16', 'bf16') else 'f32')
        # (single-product convolutions only where `auto` has measured them: AUTO_CANDIDATES -- or, on the OSG path, where the caller asked for a
        #  single-product precision: its head is fp32 in every case, so there the setting is about the tables and the encoder alone)
        enc = enc if enc != 'auto' else ('f16' if not self.use_NeRF_decoder and mlp in ('f16', 'bf16') else 'f16x3')
        return (mlp, tab, enc), False

    def _set_config(self, fr, decoder, dev, cfg, exact):
        """The precision-dependent fields of the frame descriptor: the MLP fragment stream and the table / encoder flags."""
        wc = self._weights(decoder, dev, cfg[0])
        fr.wstream, fr.wbias = _lib.addr(wc['stream']), _lib.addr(wc['wbias'])
        fr.mlp_prec = MLP_PRECISIONS[cfg[0]] | (0 if self.use_trans else _lib.MLP_NO_TRANSFORMER)
        fr.flags = (1 if exact else 0) | (2 if cfg[1] == 'f16' else 0) | (4 if cfg[2] == 'f16' else 0) | (16 if self.__dict__.get('_opt_report_count') else 0)
        if not self.use_NeRF_decoder:
            # OSG path (sherf_osg_decoder): one launch form -- mlp_form / mlp_split / pe_in_gather do not apply and the form tuner never runs
            fr.mlp_prec |= _lib.MLP_OSG_DECODER
            fr.zfrag = fr.pefrag = None
            self.__dict__['_form_auto'] = False
            return wc
        # the two-launch form of the per-sample network (csrc/mlp.hip: nerf_tokens_kernel + nerf_decoder_kernel, bit-identical results):
        # opt-in.  Measured SLOWER than the one-launch kernel on the MI355X in every precision (f16, 512x512x64: 0.35 vs 0.285 ms at 4 %
        # valid samples, 0.62 vs 0.51 ms at 7.6 %; profiles/r04_call_b_mlp_ablations.txt) -- see csrc/mlp.hip for why
        split = getattr(self, '_opt_mlp_split', None)
        if split is None:
            split = bool(getattr(self, 'mlp_split', None))
        form = getattr(self, '_opt_mlp_form', None) or getattr(self, 'mlp_form', 'auto')
        if form not in ('auto', 'pipelined', 'two_tiles', 'one'):
            raise ValueError(f"mlp_form must be 'auto', 'pipelined', 'two_tiles' or 'one', not {form!r}")
        self.__dict__['_form_auto'] = form == 'auto'
        if form == 'auto':
            form = self._FORM_CHOICE.get(self._form_key(dev, cfg[0], fr), 'pipelined')
        if cfg[0] != 'f16x3' and not split:
            fr.flags |= {'pipelined': 64, 'two_tiles': 32, 'one': 0}[form]   # SHERF_FRAME_MLP_PIPELINED / SHERF_FRAME_MLP_TWO_TILES
        fr.zfrag = None
        if split:
            ws = self._workspace(dev)
            fr.zfrag = _lib.addr(ws.zfrag(int(fr.tok_capacity or fr.capacity), cfg[0], dev))
            fr.flags |= 8
        # round 6: the positional encodings leave the power-bound network kernel for the latency-bound gather (SHERF_FRAME_PE_FRAGS; the frame
        # driver ignores the flag outside the configuration it is built for: fp16 tables, single fp16 products, the pipelined form, one part)
        # MEASURED (MI355X, profiles/r06_call_a_*): bit-identical frames; the network kernel 0.509 -> 0.496 ms (-2.4 %; alone on the frame's tokens:
        # 0.526 -> 0.523), the gather 0.463 -> 0.602 ms: the frame LOSES 0.14 ms.  Opt-in (rendering option / attribute `pe_in_gather`,
        # SHERF_PE_IN_GATHER=1), off by default.
        pe = getattr(self, '_opt_pe_in_gather', None)
        if pe is None:
            pe = getattr(self, 'pe_in_gather', os.environ.get('SHERF_PE_IN_GATHER', '0') == '1')
        fr.pefrag = None
        if pe and cfg[0] == 'f16' and cfg[1] == 'f16' and form == 'pipelined' and not split:
            fr.pefrag = _lib.addr(self._workspace(dev).pefrag(dev))
            fr.flags |= 128
        return wc

    _FORM_CHOICE = {}                   # (device, precision, size class) -> the fastest of the bit-identical launch forms on THIS board (process-wide)

    @staticmethod
    def _form_key(dev, prec_name, fr):
        """The tuner's key: the board, the precision and the frame's size class (token capacity in factors of four) -- a process whose first frame is a thumbnail does
        not decide for its full-size frames."""
        cap = int(fr.tok_capacity or fr.capacity or 1)
        return (str(dev), prec_name, max(cap, 1).bit_length() // 2)

    _FORM_ENTRY = dict(pipelined='sherf_nerf_mlp3', two_tiles='sherf_nerf_mlp2', one='sherf_nerf_mlp')

    def _tune_mlp_form(self, fr, ws, dev, prec_name, levels, streams):
        """mlp_form='auto': time WHOLE FRAMES in each of the three bit-identical launch forms of the single-product network -- the frame just rendered, again (same
        descriptor but the form bits; every form rewrites the same outputs with the same bits; the encoder's running statistics are not advanced: that is finish()) --
        and keep the fastest for this (device, precision).  Whole frames, not the kernel alone: under the board's power cap the kernel runs ~15 % faster behind the
        frame's low-power first phase than back to back, and the forms' ranking differs between the two settings (profiles/r06_y_*: in the frame pipelined beats the
        one-tile kernel, back to back it loses to it).  Interleaved rounds, HIP events on the caller's stream: 36 frames, once per process and board."""
        key = self._form_key(dev, prec_name, fr)
        if key in self._FORM_CHOICE or dev.type != 'cuda' or prec_name not in ('f16', 'bf16'):
            return
        st = torch.cuda.current_stream(dev)
        keep = int(fr.flags)
        base = keep & ~(32 | 64 | 128 | 16)            # (the form bits, the encodings-in-gather form tied to one of them, the per-frame count report)
        bits = dict(pipelined=64, two_tiles=32, one=0)
        times = {f: [] for f in bits}
        frame = lambda: _lib.call('sherf_render_frame', _ct.byref(fr), 3, levels, *streams)
        try:
            for rnd in range(3):                       # (round 0 warms up)
                for form, b in bits.items():
                    fr.flags = base | b
                    frame()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    for _ in range(3):
                        frame()
                    e1.record(st)
                    e1.synchronize()
                    if rnd:
                        times[form].append(e0.elapsed_time(e1) / 3)
        finally:
            fr.flags = keep
        ms = {f: min(v) for f, v in times.items()}
        best = min(ms, key=ms.get)
        self._FORM_CHOICE[key] = best
        self.__dict__['form_report'] = dict(choice=best, ms={k: round(v, 4) for k, v in ms.items()}, basis='ms per whole frame, best of 2 interleaved rounds of 3 frames',
                                            device=str(dev), precision=prec_name)

    def _calibrate(self, fr, decoder, dev, ws, levels, streams, exact):
        """mlp_precision='auto': before the frame proper (the reference configuration) the SAME frame is rendered in every candidate
        configuration and its per-sample sigma+ / rgb are kept; the first (cheapest) candidate within AUTO_TOL -- true relative error
        with the parity floors, EVERY sample of the frame -- of the reference result is used from the next frame on.  One extra frame
        per candidate and one host wait, once per set of weights."""
        cands = []
        for cfg in self.AUTO_CANDIDATES:
            self._set_config(fr, decoder, dev, cfg, exact)
            _lib.call('sherf_render_frame', _ct.byref(fr), 1, levels, *streams)
            cands.append((cfg, ws['sample_out'].clone()))
        self._set_config(fr, decoder, dev, self.REFERENCE_CONFIG, exact)
        softplus = bool(int(fr.white_back) & _lib.COMPOSITE_SOFTPLUS)

        def decide():
            ref = ws['sample_out']
            nv = int(ws['counters'][0])
            choice, report = self.REFERENCE_CONFIG, {}
            if nv > 0:
                # the density the compositing kernel forms from sigma: relu, or softplus(sigma - 1) (a negative sigma counts there)
                act = (lambda x: torch.nn.functional.softplus(x - 1)) if softplus else (lambda x: x.clamp(min=0))
                sig_r = act(ref[:nv, 3])
                for cfg, out in cands:
                    e_sig = ((act(out[:nv, 3]) - sig_r).abs() / sig_r.clamp(min=1.0)).max()
                    e_rgb = ((out[:nv, :3] - ref[:nv, :3]).abs() / ref[:nv, :3].abs().clamp(min=0.1)).max()
                    e = float(torch.maximum(e_sig, e_rgb))
                    report['mlp %s / tables %s / encoder %s' % cfg] = e
                    if e == e and e <= self.AUTO_TOL:
                        choice = cfg
                        break
            wc = self._wcache
            wc['auto'] = choice
            wc['auto_key'], wc['auto_frames'], wc['auto_tripped'] = self._auto_state_key(), 0, (self.__dict__.get('_flags') or {}).get('tripped', 0)
            self.auto_report = dict(choice=choice[0], config=dict(mlp=choice[0], tables=choice[1], encoder=choice[2]),
                                    errors_vs_reference_config=report, samples=nv, tol=self.AUTO_TOL,
                                    recheck_every_frames=self.AUTO_RECHECK_EVERY, recalibrations=list(wc.get('auto_recalibrations', [])))
            return choice
        return decide

    # ---- reuse of the encoded observation across the frames of a sweep ---------------------------------------------------------
    def _observation_key(self, wsp, wc, pl, cfg, planes, obs_input_feature, obs_input_img, sp, obs_sp_input, tables):
        """-> (key, refs): everything the folded tables (planes_f / feat_f / img4) and the plan's voxel levels are a function of.  Two frames with equal
        keys on one workspace fold and encode the same bits, so the second may render from what the first left (csrc/frame.hip,
        SHERF_FRAME_REUSE_OBSERVATION).  Input tensors by identity, address and version counter; the weights through the caches that already track
        them -- `_weights` (the projections behind Wa_t / Wb_t / the fold matrices / tok_bias), the encoder's packed weights and its plan, in eval mode
        the running statistics `prepare` folded into the plan; the resolved table / encoder precision and the encoder's mode; the buffers themselves.
        `refs` keeps every keyed tensor alive while the key is recorded: a freed address cannot come back at version 0 and compare equal.
        (A write that does not bump `_version` -- through a raw pointer, `.data`, another process -- cannot be seen: INTEGRATION.md.)"""
        ident = lambda t: (id(t), t.data_ptr(), t._version)
        enc = self.encoder_3d
        inputs = (planes, obs_input_feature, obs_input_img, sp.features, sp.indices, obs_sp_input['bounds'])
        packed = (wc['Wa_t'], wc['Wb_t'], wc['tok_bias']) + tuple(wc['fold'])
        key = (id(self), tuple([ident(t) for t in inputs]), tuple([int(v) for v in obs_sp_input['out_sh']]),
               wc['key'], tuple([ident(t) for t in packed]),
               id(pl), pl['key'], None if enc.training else pl.get('eval_key'), bool(enc.training), cfg[1], cfg[2],
               id(wsp.t), tuple([(t.data_ptr(), tuple(t.shape)) for t in tables]))
        return key, (inputs, packed, pl, tables, wsp.t)

    def observation_stats(self):
        """(frames of this renderer that encoded their observation, frames that reused it): rendering option `reuse_observation`."""
        st = self.__dict__.get('_obs_stats') or (0, 0)
        return int(st[0]), int(st[1])

    def _describe(self, wsp, wc, planes, obs_input_img, obs_input_feature, canonical_sp_conv_volume, obs_sp_input, input_data, opts, dev, keep):
        """The part of the `sherf_frame` descriptor that does not depend on what is sampled -- SMPL parameter sets, cameras, vertices, the folded tables, the
        gather's switches, the encoder plan and this call's voxels, the streams -- for `forward` (rays) and `query_points` (points) alike.
        -> (descriptor, dict of what the callers go on with).  Only collects pointers; conversions that must outlive the enqueue go to `keep`."""
        F32 = torch.float32

        def f32(t):                                    # (already fp32 and contiguous -- the usual case: no dispatcher round trips)
            return t if (t.dtype is F32 and t.is_contiguous() and not t.requires_grad) else t.detach().to(dtype=F32).contiguous()
        smpl = self._smpl(dev)
        prm, oprm, tprm = input_data['params'], input_data['obs_params'], input_data['t_params']
        main = torch.cuda.current_stream(dev)
        side = self._side(dev)
        A = _lib.addr
        fr = wsp.descriptor(smpl)                                        # workspace / asset pointers: filled in once per workspace

        def a32(t, n):                                                   # address of `t` as n contiguous fp32 values
            t = f32(t)
            if t.numel() != n:
                raise RuntimeError(f'sherf_amd: expected {n} values, got a tensor of shape {tuple(t.shape)}')
            keep.append(t)
            return A(t)

        # the three SMPL parameter sets side by side (target, big pose, observation): two small concatenations per frame -- reused while
        # the six source tensors are the same objects at the same versions (a static subject / camera sweep)
        srcs = (prm['poses'], tprm['poses'], oprm['poses'], prm['shapes'], tprm['shapes'], oprm['shapes'])
        skey = tuple([(id(t), t._version, t.data_ptr()) for t in srcs])
        if wsp.stacked is None or wsp.stacked[0] != skey:
            # (written into the SAME two tensors every time: their addresses are part of the frame graph's key, csrc/frame.hip)
            old = wsp.stacked
            po = old[1] if old is not None and old[1].device == dev else torch.empty(3, 72, dtype=F32, device=dev)
            sh = old[2] if old is not None and old[2].device == dev else torch.empty(3, 10, dtype=F32, device=dev)
            torch.stack([f32(t).reshape(72) for t in srcs[:3]], out=po)
            torch.stack([f32(t).reshape(10) for t in srcs[3:]], out=sh)
            wsp.stacked = (skey, po, sh, srcs)
        poses, shapes = wsp.stacked[1], wsp.stacked[2]
        fr.poses, fr.shapes = A(poses), A(shapes)
        nl = wsp.desc[3]
        if opts.get('near_lists', getattr(self, 'near_lists', True)):           # exact vertex list per near-mask sub-cell (False: the cell walk)
            fr.near_hdr, fr.near_list, fr.near_list_cap = nl['near_hdr'], nl['near_list'], nl['near_cap']
        else:
            fr.near_hdr, fr.near_list, fr.near_list_cap = None, None, 0
        fr.obs_R, fr.obs_Th = a32(oprm['R'], 9), a32(oprm['Th'], 3)
        fr.cam_R, fr.cam_T, fr.cam_K = a32(input_data['obs_R_all'], 9), a32(input_data['obs_T_all'], 3), a32(input_data['obs_K_all'], 9)
        fr.verts, fr.tverts = a32(input_data['vertices'], V * 3), a32(input_data['t_vertices'], V * 3)
        fr.Rg, fr.Th = a32(prm['R'], 9), a32(prm['Th'], 3)
        # per-frame table re-layout (channel-last) with the slot projections folded in
        Pres = planes.shape[-1]
        Hf, Wf = obs_input_feature.shape[-2:]
        H, W = obs_input_img.shape[-2:]
        planes_f = wsp.table('planes_f', (3, Pres, Pres, 32), dev)
        feat_f = wsp.table('feat_f', (Hf, Wf, 64), dev)
        img4 = wsp.table('img4', (H, W, 4), dev)
        fr.planes, fr.Wa_t, fr.planes_f, fr.P = a32(planes, planes.numel()), A(wc['Wa_t']), A(planes_f), Pres
        fr.obs_feat, fr.Wb_t, fr.feat_f, fr.Hf, fr.Wf = a32(obs_input_feature, obs_input_feature.numel()), A(wc['Wb_t']), A(feat_f), Hf, Wf
        fr.obs_img, fr.img4, fr.H, fr.W = a32(obs_input_img, obs_input_img.numel()), A(img4), H, W
        fr.tok_bias, fr.bounds = A(wc['tok_bias']), a32(input_data['t_world_bounds'], 6)
        vox_min = f32(obs_sp_input['bounds'])                            # [.., 2, 3]: its first row = the voxel grid's origin
        if vox_min.numel() != 6:
            raise RuntimeError('sherf_amd: obs_sp_input["bounds"] must hold 2 x 3 values')
        keep.append(vox_min)
        fr.vox_min = A(vox_min)
        for i, v in enumerate(obs_sp_input['out_sh']):
            fr.vox_sh[i] = int(v)
        gb = opts.get('gather_branchless', self.gather_branchless)
        fr.gather_split = (1 if opts.get('gather_split', self.gather_split) else 0) | (4 if gb == '128' else 2 if gb else 0)
        # a11: sparse voxel encoder plan (persistent buffers) + this frame's voxels
        pl, vfeat, vcoord = self.encoder_3d.prepare(canonical_sp_conv_volume, wc['fold'], wsp)
        keep += [vfeat, vcoord]
        fr.vox_plan = _ct.addressof(pl['plan'])
        fr.vox_coord, fr.vox_feat, fr.vox_n, fr.vox_training = A(vcoord), A(vfeat), vfeat.shape[0], 1 if self.encoder_3d.training else 0
        levels = (_lib.VoxLevel * 3)()
        s_main, s_side = _ct.c_void_p(main.cuda_stream), _ct.c_void_p(side.cuda_stream)
        s_aux = _ct.c_void_p(self._side(dev, 1).cuda_stream) if opts.get('aux_stream', self.aux_stream) else None
        return fr, dict(a32=a32, pl=pl, planes_f=planes_f, feat_f=feat_f, img4=img4, vox_min=vox_min, vcoord=vcoord, H=H, W=W, levels=levels,
                        streams=(s_main, s_side, s_aux))

    # ---- forward -----------------------------------------------------------------------------
    def forward(self, planes, obs_input_img, obs_input_feature, canonical_sp_conv_volume, obs_smpl_vertex_mask, obs_sp_input,
                decoder, ray_origins, ray_directions, near, far, input_data, rendering_options):
        n_imp = int(rendering_options.get('depth_resolution_importance', 0) or 0)
        if n_imp != 0 and ((getattr(self, 'enable_autograd', False) and torch.is_grad_enabled()) or getattr(self, '_in_autograd', False)):
            raise NotImplementedError('depth_resolution_importance > 0 in a grad-recorded forward (enable_autograd with grad enabled): the backward through '
                                      'the fine samples is not built; render under torch.no_grad() or train with depth_resolution_importance = 0')
        if getattr(self, 'enable_autograd', False) and torch.is_grad_enabled() and not getattr(self, '_in_autograd', False):
            if not self.use_NeRF_decoder and not getattr(self, 'enable_osg_autograd', False):
                raise NotImplementedError('the backward of the OSG path (use_NeRF_decoder=False: OSGDecoder, sherf_osg_decoder / sherf_bwd_osg_head) is staged: '
                                          'with enable_autograd alone this renderer is forward-only; set enable_osg_autograd = True beside it to train through it')
            # opt-in training path (BASELINE config 5): the same forward, recorded as one autograd node whose backward runs
            # the HIP backward pipeline (sherf_amd/backward.py; experimental until verified on hardware).  Every combination of the feature-branch
            # switches trains: the backward leaves the absent branches out (backward.py: render_backward)
            from .backward import RenderFunction, _named_params

            def call():
                self._in_autograd = True
                self.encoder_3d._force_stats_update = True      # a training forward updates the BatchNorm running statistics
                try:
                    return self.forward(planes, obs_input_img, obs_input_feature, canonical_sp_conv_volume, obs_smpl_vertex_mask,
                                        obs_sp_input, decoder, ray_origins, ray_directions, near, far, input_data, rendering_options)
                finally:
                    self._in_autograd = False
                    self.encoder_3d._force_stats_update = False
            return RenderFunction.apply(self, decoder, call, planes, obs_input_feature, canonical_sp_conv_volume.features,
                                        *[p for _, p in _named_params(self, decoder)])
        self._check_decoder(decoder)
        if not ray_origins.is_cuda:
            raise RuntimeError('sherf_amd.ImportanceRenderer runs on the GPU only (no CPU fallback)')
        if ray_origins.shape[0] != 1:
            raise RuntimeError('per-GPU batch must be 1, as in the reference (renderer.py:320-321,567)')
        opts = rendering_options
        if ray_origins.device.index is not None and ray_origins.device.index != torch.cuda.current_device():
            # the native frame driver keeps per-device state under hipGetDevice() and the helpers use the current stream: render
            # under the tensors' device
            with torch.cuda.device(ray_origins.device):
                return self.forward(planes, obs_input_img, obs_input_feature, canonical_sp_conv_volume, obs_smpl_vertex_mask, obs_sp_input,
                                    decoder, ray_origins, ray_directions, near, far, input_data, rendering_options)
        if n_imp != 0:
            self._check_importance(opts, n_imp, ray_origins.shape[1])
        if opts.get('disparity_space_sampling', False):
            raise NotImplementedError('only disparity_space_sampling=False (train.py:330-332)')
        _lib.composite_bits(False, opts.get('clamp_mode', 'relu'))     # 'relu' / 'softplus'; anything else: the reference marcher's assertion (ray_marcher.py:41-42)
        # the state keys of the weights are computed once in this call (see _weights, _auto_state_key, SparseConvNet._pack); plain
        # __dict__ stores: nn.Module.__setattr__ costs more than the walks it would guard
        d, enc = self.__dict__, self.encoder_3d.__dict__
        d['_frame_memo'] = (None, None, None)
        enc['_key_memo'] = state_key(fast_params(self.encoder_3d))
        try:
            if n_imp != 0:                                 # the two-pass frame: inference only, nothing is recorded
                with torch.no_grad():
                    return self._forward(planes, obs_input_img, obs_input_feature, canonical_sp_conv_volume, obs_sp_input, decoder, ray_origins,
                                         ray_directions, near, far, input_data, opts)
            return self._forward(planes, obs_input_img, obs_input_feature, canonical_sp_conv_volume, obs_sp_input, decoder, ray_origins,
                                 ray_directions, near, far, input_data, opts)
        finally:
            d['_frame_memo'] = None
            enc['_key_memo'] = None

    # ---- importance sampling (depth_resolution_importance = N > 0): csrc/importance.hip, csrc/frame.hip: sherf_render_frame_importance ----
    def _check_importance(self, opts, N, R):
        """What the two-pass frame refuses, each by the option's name, before anything is enqueued."""
        S = int(opts['depth_resolution'])
        if N < 1 or N > 256:
            raise ValueError(f'depth_resolution_importance must be within 0..256, got {N}')
        if S < 3 or S > 256:
            raise ValueError(f'depth_resolution must be within 3..256 when depth_resolution_importance > 0, got {S} '
                             '(2 coarse samples leave weights[:, 1:-1] empty in the reference)')
        if float(opts.get('density_noise', 0) or 0) > 0:
            raise NotImplementedError('density_noise > 0 with depth_resolution_importance > 0 is not built (the noise is a training option; the two-pass frame is inference only)')
        if opts.get('depth_range') is not None:
            raise NotImplementedError('depth_range (the ray-tile sharding of sherf_amd.dist) with depth_resolution_importance > 0 is not built')
        u = opts.get('importance_u')
        if u is not None:
            if not torch.is_tensor(u) or u.dtype != torch.float32 or tuple(u.shape) not in ((R, N), (1, R, N)):
                raise ValueError(f'importance_u must be a float32 tensor of shape [{R}, {N}] or [1, {R}, {N}], got '
                                 f'{tuple(u.shape) if torch.is_tensor(u) else type(u).__name__}' + (f' of {u.dtype}' if torch.is_tensor(u) else ''))
            if not bool(((u >= 0) & (u <= 1)).all()):      # (NaN fails both comparisons)
                raise ValueError('importance_u must lie within [0, 1]')

    def _importance_workspace(self, wsp, R, N, dev):
        """The fine pass's own buffers, kept in the frame's workspace (dropped with it when the frame's shape changes): the point sampler's for R * N points
        laid out as rows of 64 and the fine depths / positions; the token side is sized by `_importance_tokens`."""
        fw = wsp.t.get('fine')
        if fw is not None and fw['key'] == (R, N):
            return fw
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        rows = (R * N + 63) // 64
        cap = rows * 64
        fw = dict(key=(R, N), rows=rows, capacity=cap, tok_cap=0,
                  counters=torch.zeros(8, **i32), ray_base=torch.zeros(rows, **i32), ray_cnt=torch.zeros(rows, **i32), cs_idx=torch.zeros(cap, **i32),
                  cs_vid=torch.zeros(cap, **i32), cs_xs=torch.zeros(cap, 4, **f32), dense_vid=torch.zeros(cap, **i32),
                  ray_mask=torch.zeros(rows, dtype=torch.int64, device=dev), scan_ws=torch.zeros(rows + rows // 1024 + 2, **i32),
                  depths_fine=torch.zeros(R, N, **f32), points=torch.zeros(cap, 3, **f32))
        wsp.t['fine'] = fw
        return fw

    @staticmethod
    def _importance_tokens(fw, tok_cap, dev):
        """The fine pass's token-side buffers (what _Workspace.tokens holds for the coarse pass) for `tok_cap` samples."""
        if tok_cap == fw['tok_cap']:
            return
        f32 = dict(dtype=torch.float32, device=dev)
        tiles = (tok_cap + 31) // 32 + 8
        for k in ('geom', 'tokens', 'extras', 'sample_out', 'cs_tvid'):
            fw.pop(k, None)
        fw.update(geom=torch.zeros(tok_cap, 8, **f32), tokens=torch.zeros(tiles * 3 * 8 * 32 * 4, **f32), extras=torch.zeros(tiles * 12 * 32, **f32),
                  sample_out=torch.zeros(tok_cap, 4, **f32), cs_tvid=torch.zeros(tok_cap, dtype=torch.int32, device=dev), tok_cap=tok_cap)

    def _importance_descriptor(self, fw, u, N):
        A = _lib.addr
        im = _lib.Importance()
        im.n, im.u, im.depths_fine, im.points = N, (None if u is None else A(u)), A(fw['depths_fine']), A(fw['points'])
        im.capacity, im.tok_capacity = fw['capacity'], fw['tok_cap']
        for k in ('counters', 'ray_base', 'ray_cnt', 'cs_idx', 'cs_vid', 'cs_xs', 'dense_vid', 'ray_mask', 'scan_ws', 'geom', 'cs_tvid', 'tokens', 'extras',
                  'sample_out'):
            setattr(im, k, A(fw[k]))
        return im

    def _forward(self, planes, obs_input_img, obs_input_feature, canonical_sp_conv_volume, obs_sp_input, decoder, ray_origins,
                 ray_directions, near, far, input_data, opts):
        dev = ray_origins.device
        S = int(opts['depth_resolution'])
        R = ray_origins.shape[1]
        cap = int(opts.get('sample_capacity', R * S))
        clamp_mode = opts.get('clamp_mode', 'relu')
        self.__dict__['_clamp_mode'] = clamp_mode                        # (part of what an `auto` choice was measured under: _auto_state_key)
        cfg, calibrate = self._resolve_config(opts, decoder, dev)
        self.__dict__['_opt_mlp_split'] = opts.get('mlp_split')
        self.__dict__['_opt_mlp_form'] = opts.get('mlp_form')
        self.__dict__['_opt_pe_in_gather'] = opts.get('pe_in_gather')
        prec_name = cfg[0]
        wc = self._weights(decoder, dev, prec_name)
        wsp = self._workspace(dev)
        ws = wsp.frame(R, S, cap, dev)
        prm = input_data['params']
        # One native call enqueues the whole frame on two HIP streams (csrc/frame.hip): the sparse voxel encoder is a chain
        # of ~35 small launches that cannot fill the chip and is independent of the ray side of the frame until the
        # gather -> it runs (with the SMPL tables) on a side stream, concurrently with cell lists / sampling / compaction /
        # table folding on the caller's stream.  Everything below only collects pointers.
        A = _lib.addr
        keep = []                                                        # conversions that must outlive the enqueue
        fr, ob = self._describe(wsp, wc, planes, obs_input_img, obs_input_feature, canonical_sp_conv_volume, obs_sp_input, input_data, opts, dev, keep)
        a32 = ob['a32']
        pl, planes_f, feat_f, img4, vox_min, vcoord, H, W = ob['pl'], ob['planes_f'], ob['feat_f'], ob['img4'], ob['vox_min'], ob['vcoord'], ob['H'], ob['W']
        levels, (s_main, s_side, s_aux) = ob['levels'], ob['streams']
        # the frame's outputs: ONE fresh buffer per call, planar [rgb (3R) | depth (R) | acc (R)], written by the compositing kernel and
        # returned as views -- no copies behind the frame (rounds 1-2 cloned three workspace tensors: three launches per frame), and
        # a caller may keep as many frames as it likes
        # Round 6: frames can replay as hipGraphs (csrc/frame.hip; opt-in, SHERF_FRAME_GRAPH=1 -- measured: no GPU-side gain), keyed on every pointer
        # of the descriptor -- then the compositing kernel writes a buffer OWNED BY THE WORKSPACE (the same address frame after frame) and the
        # caller's fresh buffer is one copy behind the frame (5 R floats: ~3 us); otherwise the kernel writes the fresh buffer itself
        static_out = dev.type == 'cuda' and os.environ.get('SHERF_FRAME_GRAPH', '0') == '1'
        if static_out:
            out = wsp.t.get('out_static')
            if out is None or out.numel() != 5 * R or out.device != dev:
                out = wsp.t['out_static'] = torch.empty(5 * R, dtype=torch.float32, device=dev)
        else:
            out = torch.empty(5 * R, dtype=torch.float32, device=dev)
        fr.rgb, fr.depth, fr.acc = A(out), A(out) + 12 * R, A(out) + 16 * R
        fr.ray_o, fr.ray_d = a32(ray_origins, R * 3), a32(ray_directions, R * 3)
        fr.near, fr.far = a32(near, R), a32(far, R)
        fr.R, fr.S, fr.capacity = R, S, cap
        exact = bool(opts.get('exact_grids', self.exact_grids))

        # token-side workspace: sized from the frame's own count (see _token_capacity)
        def probe():
            _lib.call('sherf_render_frame', _ct.byref(fr), 4, levels, s_main, s_side, s_aux)
            return int(ws['counters'][0])                                # (one host wait, once per workspace)
        first = wsp.__dict__.get('nv_sized_for') is None
        tok = self._token_capacity(opts, wsp, cap, dev, probe)
        # a frame whose rays / vertices are not the previous frame's tensors may hold any number of valid samples: its count is read back
        # right behind the sampler (the rest of the frame stays in flight) and the frame is rendered again if it did not fit.  Frames on the
        # same inputs (a benchmark loop) and slowly changing sequences on explicit / worst-case capacities never wait.
        # (everything the count depends on: the posed vertices, the rays' origins AND directions, the depth range, the global rotation /
        #  translation of the SMPL frame.  The keyed tensors are kept referenced so that a freed tensor's address cannot come back at
        #  version 0 and compare equal -- ADVICE round 4)
        keyed = (input_data['vertices'], ray_origins, ray_directions, near, far, prm['R'], prm['Th'])
        scene = tuple(x for t in keyed for x in (t.data_ptr(), t._version))
        verify = (not first and wsp.__dict__.get('scene') != scene and wsp.tok_cap < cap
                  and opts.get('token_capacity', getattr(self, 'token_capacity', 'auto')) == 'auto' and tok < cap)
        wsp.scene = scene
        wsp.scene_refs = keyed
        self.__dict__['_opt_report_count'] = verify
        if tok != wsp.tok_cap:
            if dev.type == 'cuda' and not isinstance(ws['counters'], type(None)) and ws['counters'].device.type == 'cuda':
                torch.cuda.synchronize(dev)                              # frames in flight still read the old buffers
            wsp.tokens(tok, dev)
        fr.tok_capacity = wsp.tok_cap
        # a13-a14: fused transformer + NeRF decoder
        self._set_config(fr, decoder, dev, cfg, exact)
        fr.mlp_parts = int(opts.get('mlp_parts', getattr(self, 'mlp_parts', 0)))
        fr.white_back = _lib.composite_bits(opts.get('white_back', False), clamp_mode)     # bit 0: white background, bit 1: softplus
        fr.main_after_layer = int(opts.get('main_after_layer', self.main_after_layer))
        noise = float(opts.get('density_noise', 0) or 0)
        # rendering option `reuse_observation`: the native flag is set only when this frame's observation key equals the one the workspace recorded
        # for what its tables and voxel levels hold; any difference encodes as always and records the new key.  Never for a grad-recorded forward
        # (its backward reads this frame's own tables) nor for a calibration frame of mlp_precision='auto' (it renders through other precisions).
        recorded = (torch.is_grad_enabled() and getattr(self, 'enable_autograd', False)) or getattr(self, '_in_autograd', False)
        want_reuse = bool(opts.get('reuse_observation', getattr(self, 'reuse_observation', False))) and not recorded
        obs_key = obs_refs = None
        reused = False
        if want_reuse:
            obs_key, obs_refs = self._observation_key(wsp, wc, pl, cfg, planes, obs_input_feature, obs_input_img, canonical_sp_conv_volume, obs_sp_input,
                                                      (planes_f, feat_f, img4))
            reused = not calibrate and wsp.obs_key is not None and wsp.obs_key == (obs_key, wsp.tok_cap)
        if reused:
            fr.flags |= _lib.FRAME_REUSE_OBSERVATION
            levels = wsp.obs_levels                                      # an INPUT of the native call under the flag: the encoding frame's array
        else:
            wsp.obs_key = None                                           # (until this frame's own encode has been enqueued)
        decide = None
        if calibrate and noise == 0:
            decide = self._calibrate(fr, decoder, dev, ws, levels, (s_main, s_side, s_aux), exact)
        rng = opts.get('depth_range')                                    # sherf_amd.dist: [lo, hi] of the WHOLE frame's depths
        # depth_resolution_importance = N > 0: the two-pass frame (one native call: coarse phase 1, the fine depths, the fine pass on its own buffers, the
        # merged compositing).  The draws: rendering option `importance_u`, else torch.rand from the global generator -- where sample_pdf draws them.
        n_imp = int(opts.get('depth_resolution_importance', 0) or 0)
        fw = im = imp_u = None
        if n_imp > 0:
            fw = self._importance_workspace(wsp, R, n_imp, dev)
            given = opts.get('importance_depths')                        # TEST ONLY: the fine depths [R, N] themselves (ascending per ray) instead of draws
            if given is not None:
                fw['depths_fine'].copy_(given.reshape(R, n_imp))
                imp_u = None
            else:
                imp_u = opts.get('importance_u')
                imp_u = torch.rand(R, n_imp, device=dev) if imp_u is None else imp_u.reshape(R, n_imp).contiguous()
                keep.append(imp_u)
            # the fine token buffers follow the frame's token_capacity policy on their OWN count: 'worst' = a row per fine sample, a number as given,
            # 'auto' = what the workspace's last importance frame needed (a first frame starts small and is rendered again once its count is known)
            want = opts.get('token_capacity', getattr(self, 'token_capacity', 'auto'))
            ftok = fw['capacity'] if want in ('worst', None) else (fw['tok_cap'] or self._round_tokens(0, fw['capacity'])) if want == 'auto' \
                else self._round_tokens(int(want), fw['capacity'])
            if ftok != fw['tok_cap']:
                if dev.type == 'cuda' and fw['counters'].device.type == 'cuda':
                    torch.cuda.synchronize(dev)
                self._importance_tokens(fw, ftok, dev)
            im = self._importance_descriptor(fw, imp_u, n_imp)
            fr.flags |= 16                                               # SHERF_FRAME_REPORT_COUNT: both counts are checked behind the fine pass's sampler
            verify = False                                               # (the check below covers the coarse count as well)

        def enqueue():
            if im is not None:
                _lib.call('sherf_render_frame_importance', _ct.byref(fr), _ct.byref(im), levels, s_main, s_side, s_aux)
                return
            if noise > 0 or rng is not None:
                _lib.call('sherf_render_frame', _ct.byref(fr), 1, levels, s_main, s_side, s_aux)
                if noise > 0:                                            # renderer.py:435-436 (training only)
                    ws['sample_out'][:, 3] += torch.randn(wsp.tok_cap, device=dev) * noise
                if rng is not None:
                    # ray_marcher.py:57 clamps the depth image with the min / max over ALL depths of the frame; when this call renders
                    # only a subset of the frame's rays (ray-tile sharding) the caller supplies the frame-wide range, which replaces
                    # the subset's own in the counters the compositing kernel reads (order-preserving int encoding, csrc/common.h: f2ord)
                    bits = torch.as_tensor(rng, dtype=torch.float32, device=dev).reshape(2).contiguous().view(torch.int32)
                    ws['counters'][1:3] = torch.where(bits >= 0, bits, bits ^ 0x7FFFFFFF)
                _lib.call('sherf_render_frame', _ct.byref(fr), 2, levels, s_main, s_side, s_aux)
            else:
                _lib.call('sherf_render_frame', _ct.byref(fr), 3, levels, s_main, s_side, s_aux)
        enqueue()
        if verify:
            nv_now = _ct.c_int32(0)
            _lib.call('sherf_frame_count', _ct.byref(nv_now))            # waits for this frame's sampler only
            if nv_now.value > wsp.tok_cap:
                if dev.type == 'cuda' and ws['counters'].device.type == 'cuda':
                    torch.cuda.synchronize(dev)
                wsp.tokens(self._round_tokens(self.TOKEN_HEADROOM * nv_now.value, cap), dev)
                wsp.nv_sized_for = nv_now.value
                fr.tok_capacity = wsp.tok_cap
                if fr.zfrag:
                    fr.zfrag = _lib.addr(wsp.zfrag(int(fr.tok_capacity), cfg[0], dev))
                if fr.flags & 128:
                    fr.pefrag = _lib.addr(wsp.pefrag(dev))
                st = self.__dict__.setdefault('_flags', dict(ring=[], tripped=0))
                st['token_rerenders'] = st.get('token_rerenders', 0) + 1
                if decide is not None:
                    # a calibration frame that had to be rendered again on larger token buffers: the candidates' outputs were taken at the old
                    # capacity (fewer rows than this frame holds) -- drop this calibration, the next frame calibrates afresh
                    decide = None
                    self._wcache['auto'] = None
                enqueue()
        imp_counts = None
        if im is not None:
            # either list may hold more valid samples than its token buffers: re-size from the frame's own counts and render again.  The coarse count does
            # not depend on the capacities; the fine count does on the COARSE one (a ray whose coarse samples lie beyond it is resampled as empty), so the
            # worst sequence is coarse grows -> fine grows -> fits: three renders.  Every render's counts are checked; one that still does not fit fails loudly.
            # The caller never gets the overflow NaN.
            nv2 = (_ct.c_int32 * 2)()
            for attempt in range(4):
                _lib.call('sherf_importance_count', nv2)                 # waits for the fine pass's sampler only
                grow_c, grow_f = nv2[0] > wsp.tok_cap, nv2[1] > fw['tok_cap']
                if not (grow_c or grow_f):
                    break
                if attempt == 3:
                    raise RuntimeError(f'sherf_amd: the importance frame still overflows its token buffers after three re-sizes (coarse {nv2[0]} of {wsp.tok_cap}, '
                                       f"fine {nv2[1]} of {fw['tok_cap']})")
                if dev.type == 'cuda' and ws['counters'].device.type == 'cuda':
                    torch.cuda.synchronize(dev)
                st = self.__dict__.setdefault('_flags', dict(ring=[], tripped=0))
                if grow_c:
                    wsp.tokens(self._round_tokens(self.TOKEN_HEADROOM * nv2[0], cap), dev)
                    wsp.nv_sized_for = int(nv2[0])
                    fr.tok_capacity = wsp.tok_cap
                    if fr.zfrag:
                        fr.zfrag = _lib.addr(wsp.zfrag(int(fr.tok_capacity), cfg[0], dev))
                    if fr.flags & 128:
                        fr.pefrag = _lib.addr(wsp.pefrag(dev))
                    st['token_rerenders'] = st.get('token_rerenders', 0) + 1
                    if decide is not None:
                        decide = None
                        self._wcache['auto'] = None
                if grow_f:
                    self._importance_tokens(fw, self._round_tokens(self.TOKEN_HEADROOM * nv2[1], fw['capacity']), dev)
                    st['fine_token_rerenders'] = st.get('fine_token_rerenders', 0) + 1
                im = self._importance_descriptor(fw, imp_u, n_imp)
                enqueue()
            imp_counts = (int(nv2[0]), int(nv2[1]))
        if want_reuse:
            if not reused:
                wsp.obs_levels, wsp.obs_refs = levels, obs_refs
            wsp.obs_key = (obs_key, wsp.tok_cap)
        st_obs = self.__dict__.setdefault('_obs_stats', [0, 0])
        st_obs[1 if reused else 0] += 1
        if static_out:
            out = out.clone()
        if self.__dict__.get('_form_auto') and not calibrate and noise == 0 and self._form_key(dev, cfg[0], fr) not in self._FORM_CHOICE and cfg[0] != 'f16x3' \
                and not (fr.flags & 8) and int(fr.mlp_parts) <= 1 and rng is None and im is None:
            self._tune_mlp_form(fr, ws, dev, cfg[0], levels, (s_main, s_side, s_aux))    # (the frame above is complete and correct; the forms are timed behind it)
        ws['rgb'], ws['depth'], ws['acc'] = out[:3 * R].view(R, 3), out[3 * R:4 * R], out[4 * R:]
        # BatchNorm running statistics.  A grad-recorded forward follows the reference, which runs encoder_3d only under `if self.use_3d_feature`
        # (renderer.py:345-352): a renderer BUILT with use_3d_feature=False leaves every encoder_3d buffer alone (the constructor's switch, not
        # feature_branches(): (False, False, True) still runs the encoder there and uses nothing of it).  The plain no-grad forward is as it was.
        if self.use_3d_feature or not getattr(self, '_in_autograd', False):
            self.encoder_3d.finish(pl)                  # (on the encoder's own stream instead: measured, no gain -- DESIGN 9.38)
        if decide is not None:
            decide()
        if not (torch.is_grad_enabled() and getattr(self, 'enable_autograd', False)) and not getattr(self, '_in_autograd', False):
            self._flag_watch(ws, dev)                      # the frame's count and flags (non-finite fp16 operand, token overflow): no host wait
        vdbg = dict(levels=pl['L'], taps=pl['taps'], shapes=pl['shapes'])
        keep = (pl['rows'], planes_f, feat_f, img4)
        self.__dict__['last'] = dict(ws=ws, vox=vdbg, keep=keep, R=R, S=S, cap=wsp.tok_cap, sampler_cap=cap, plan=pl, levels_struct=levels, mlp_precision=cfg[0], table_precision=cfg[1], encoder_precision=cfg[2], mlp_split=bool(fr.flags & 8), mlp_form=('pipelined' if fr.flags & 64 else 'two_tiles' if fr.flags & 32 else 'one'), mlp_parts=int(fr.mlp_parts),
                                     pe_in_gather=bool(fr.flags & 128) and int(fr.mlp_parts) <= 1 and not (int(fr.gather_split) & 7),
                         # handles for the (experimental) backward, sherf_amd/backward.py: references, no copies
                         bwd=dict(planes=planes, obs_feat=obs_input_feature, ray_d=ray_directions, near=near, far=far,
                                  bounds=input_data['t_world_bounds'], vox_min=vox_min.reshape(-1)[:3], vox_sh=[int(v) for v in obs_sp_input['out_sh']],
                                  coord=vcoord, H=H, W=W, white_back=bool(opts.get('white_back', False)), clamp_mode=clamp_mode))
        self.last['out'] = out
        self.last['observation_reused'] = reused
        if im is not None:
            self.last['importance'] = dict(N=n_imp, u=imp_u, depths_fine=fw['depths_fine'], n_coarse=imp_counts[0], n_fine=imp_counts[1], ws=fw, cap=fw['tok_cap'])
        return ws['rgb'].view(1, R, 3), ws['depth'].view(1, R, 1), ws['acc'].view(1, R, 1)


    # ---- field query ---------------------------------------------------------------------------------------------------------------
    def _query_workspace(self, dev):
        """The query's own workspace per (device, caller stream): a query lays its points out as rows of 64 and sizes the sampler's buffers for them, which on the
        frames' workspace would re-size it and drop what it holds for the next frame -- its token capacity, the observation a sweep reuses, `last`."""
        q = self.__dict__.get('_qws')
        if not isinstance(q, dict):
            q = self.__dict__['_qws'] = {}
        key = (str(dev), torch.cuda.current_stream(dev).cuda_stream)
        w = q.pop(key, None)
        if w is None:
            w = _Workspace()
            while len(q) >= self.MAX_WORKSPACES:
                if dev.type == 'cuda' and torch.cuda.is_available():
                    torch.cuda.synchronize(dev)
                del q[next(iter(q))]
        q[key] = w
        return w

    def _query_config(self, opts, decoder, dev):
        """forward's precision resolution without its calibration: mlp_precision='auto' takes the choice already calibrated for these weights by a frame, else the
        fp32-grade reference configuration; the choice's frame count and re-check schedule are left alone."""
        mlp = opts.get('mlp_precision') or self.mlp_precision
        if mlp != 'auto' or not self.use_NeRF_decoder:
            return self._resolve_config(opts, decoder, dev)[0]
        self._weights(decoder, dev, 'f16x3')
        choice = self._wcache.get('auto') or self.REFERENCE_CONFIG
        tab = opts.get('table_precision') or getattr(self, 'table_precision', 'auto')
        enc = opts.get('encoder_precision') or getattr(self, 'encoder_precision', 'auto')
        return (choice[0], choice[1] if tab == 'auto' else tab, choice[2] if enc == 'auto' else enc)

    def query_stats(self):
        """Counters of this renderer's field queries: chunks issued, chunks that encoded / reused the observation, token-buffer re-sizes."""
        return dict(self.__dict__.get('_query_stats') or dict(chunks=0, encoded=0, reused=0, resizes=0))

    def query_points(self, planes, obs_input_img, obs_input_feature, canonical_sp_conv_volume, obs_smpl_vertex_mask, obs_sp_input,
                     decoder, points, directions, input_data, rendering_options):
        """Density and colour of the field at arbitrary points: `forward` from the SMPL-frame transform to the scatter-back (the reference's renderer.py:307-368)
        with `points` / `directions` [1, N, 3] -- world frame, as ray_origins / ray_directions -- in place of the ray samples and their directions; what the
        reference declares as TriPlaneGenerator.sample (triplane.py:219-230).  -> dict(rgb [1, N, 3], sigma [1, N, 1] (raw, before the clamp mode's
        activation), mask [1, N] bool: within 5 cm of a posed vertex); rgb 0 / sigma -80 where the mask fails, as colors_coarse / densities_coarse there.
        Inference only (no gradient is recorded); `density_noise` is ignored.  Same weights cache, precision resolution and launch form as `forward`
        (mlp_precision='auto': the calibrated choice if a frame has made one, else f16x3 -- a query never calibrates).  rendering_options['query_chunk']
        (default 2^24, rounded down to a multiple of 64) points go through one native call (csrc/frame.hip: sherf_query_field); the first chunk encodes the
        observation, the others reuse it.  The token buffers grow to each chunk's own count of valid points: a query never returns the overflow NaN."""
        self._check_decoder(decoder)
        if not points.is_cuda:
            raise RuntimeError('sherf_amd.ImportanceRenderer runs on the GPU only (no CPU fallback)')
        if points.shape[0] != 1:
            raise RuntimeError('per-GPU batch must be 1, as in the reference (renderer.py:320-321,567)')
        if points.ndim != 3 or points.shape[-1] != 3 or tuple(directions.shape) != tuple(points.shape) or points.shape[1] < 1:
            raise ValueError(f'points and directions must both be [1, N, 3] with N >= 1, got {tuple(points.shape)} and {tuple(directions.shape)}')
        if points.device.index is not None and points.device.index != torch.cuda.current_device():
            with torch.cuda.device(points.device):
                return self.query_points(planes, obs_input_img, obs_input_feature, canonical_sp_conv_volume, obs_smpl_vertex_mask, obs_sp_input,
                                         decoder, points, directions, input_data, rendering_options)
        d, enc = self.__dict__, self.encoder_3d.__dict__
        memo, kmemo = d.get('_frame_memo'), enc.get('_key_memo')
        d['_frame_memo'] = (None, None, None)
        enc['_key_memo'] = state_key(fast_params(self.encoder_3d))
        try:
            with torch.no_grad():
                return self._query(planes, obs_input_img, obs_input_feature, canonical_sp_conv_volume, obs_sp_input, decoder, points, directions,
                                   input_data, rendering_options)
        finally:
            d['_frame_memo'], enc['_key_memo'] = memo, kmemo

    def _query(self, planes, obs_input_img, obs_input_feature, canonical_sp_conv_volume, obs_sp_input, decoder, points, directions, input_data, opts):
        dev = points.device
        N = int(points.shape[1])
        chunk = max(64, int(opts.get('query_chunk', 1 << 24)) // 64 * 64)
        rows = (min(N, chunk) + 63) // 64
        cap = rows * 64                                                  # the sampler's buffers: a record per point of the largest chunk
        cfg = self._query_config(opts, decoder, dev)
        d = self.__dict__
        d['_opt_mlp_split'], d['_opt_pe_in_gather'] = False, False       # (opt-in forms with scratch in the frames' workspace: not for a query)
        d['_opt_mlp_form'] = opts.get('mlp_form')
        d['_opt_report_count'] = True                                    # every chunk reports its count behind the sampler
        wc = self._weights(decoder, dev, cfg[0])
        wsp = self._query_workspace(dev)
        ws = wsp.frame(rows, 64, cap, dev)
        keep = []
        fr, ob = self._describe(wsp, wc, planes, obs_input_img, obs_input_feature, canonical_sp_conv_volume, obs_sp_input, input_data, opts, dev, keep)
        a32, levels, streams = ob['a32'], ob['levels'], ob['streams']
        fr.R, fr.S, fr.capacity = rows, 64, cap
        fr.white_back = 0
        want = opts.get('token_capacity', getattr(self, 'token_capacity', 'auto'))
        tok = cap if want in ('worst', None) else wsp.tok_cap if want == 'auto' else self._round_tokens(int(want), cap)
        if tok != wsp.tok_cap:
            if dev.type == 'cuda' and ws['counters'].device.type == 'cuda':
                torch.cuda.synchronize(dev)                              # queries in flight still read the old buffers
            wsp.tokens(tok, dev)
        fr.tok_capacity = wsp.tok_cap
        self._set_config(fr, decoder, dev, cfg, bool(opts.get('exact_grids', self.exact_grids)))
        fr.mlp_parts = int(opts.get('mlp_parts', getattr(self, 'mlp_parts', 0)))
        fr.main_after_layer = int(opts.get('main_after_layer', self.main_after_layer))
        A = _lib.addr
        p_pts, p_dirs = a32(points, N * 3), a32(directions, N * 3)
        rgb = torch.empty(N, 3, dtype=torch.float32, device=dev)
        sigma = torch.empty(N, dtype=torch.float32, device=dev)
        mask = torch.empty(N, dtype=torch.uint8, device=dev)
        st = d.setdefault('_query_stats', dict(chunks=0, encoded=0, reused=0, resizes=0))
        q = _lib.FieldQuery()
        base_flags = int(fr.flags) & ~_lib.FRAME_REUSE_OBSERVATION
        counts, encoded = [], False
        for off in range(0, N, chunk):
            n = min(chunk, N - off)
            q.points, q.dirs, q.n = p_pts + 12 * off, p_dirs + 12 * off, n
            q.rgb, q.sigma, q.mask = A(rgb) + 12 * off, A(sigma) + 4 * off, A(mask) + off
            while True:
                # the first native call of this query encodes the observation; every later one -- the other chunks, a chunk issued again on larger token
                # buffers -- renders from what it left in this workspace (same inputs by construction: no key needed)
                fr.flags = base_flags | (_lib.FRAME_REUSE_OBSERVATION if encoded else 0)
                _lib.call('sherf_query_field', _ct.byref(fr), _ct.byref(q), levels, *streams)
                st['chunks'] += 1
                st['reused' if encoded else 'encoded'] += 1
                encoded = True
                nv = _ct.c_int32(0)
                _lib.call('sherf_frame_count', _ct.byref(nv))            # waits for this chunk's sampler only
                if nv.value <= wsp.tok_cap:
                    break
                if dev.type == 'cuda' and ws['counters'].device.type == 'cuda':
                    torch.cuda.synchronize(dev)
                wsp.tokens(self._round_tokens(nv.value, cap), dev)       # this chunk's own count: nothing to guess
                fr.tok_capacity = wsp.tok_cap
                st['resizes'] += 1
            counts.append(int(nv.value))
        wsp.obs_key = None                                               # (this workspace never takes part in the frames' reuse)
        d['last_query'] = dict(ws=ws, N=N, chunk=chunk, counts=counts, cap=wsp.tok_cap, keep=keep, mlp_precision=cfg[0], table_precision=cfg[1],
                               encoder_precision=cfg[2], mlp_form=('pipelined' if fr.flags & 64 else 'two_tiles' if fr.flags & 32 else 'one'))
        return dict(rgb=rgb.view(1, N, 3), sigma=sigma.view(1, N, 1), mask=mask.view(1, N).bool())
