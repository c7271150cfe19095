"""tests.bwd_emulator.EmuOps plus the entry point of the OSG path's backward (include/sherf_hip_bwd.h: sherf_bwd_osg_head), in torch on the same `Mat`
views: the test double behind tests/test_backward_osg.py.  The kernel itself is checked against float64 autograd of the head in
tests/test_hipcpu_osg_backward.py (host build) and tests/test_gpu_osg_backward.py (MI355X)."""
import torch
import torch.nn.functional as F

from tests.bwd_emulator import EmuOps


class OsgEmuOps(EmuOps):
    def osg_head(self, z, d_sample, W0g, b0g, W1g, b1g, d_z, dW0g, db0g, dW1g, db1g, max_blocks=0):      # sherf_bwd_osg_head (the four sums accumulate)
        n = z.rows
        W0, b0, W1, b1 = W0g.tensor(), b0g.tensor().view(-1), W1g.tensor(), b1g.tensor().view(-1)
        m = z.tensor().reshape(n, 3, 32).mean(1)
        a = m @ W0.t() + b0
        h = F.softplus(a)                                            # beta 1, linear above 20
        y = h @ W1.t() + b1
        s = torch.sigmoid(y[:, 1:])
        D = d_sample.tensor()
        d_y = torch.cat([D[:, 3:4], D[:, :3] * 1.002 * s * (1 - s)], 1)
        d_a = (d_y @ W1) * torch.where(a > 20, torch.ones_like(a), torch.sigmoid(a))
        d_z.tensor().copy_(((d_a @ W0) / 3).repeat(1, 3))
        dW0g.tensor().add_(d_a.t() @ m); db0g.tensor().add_(d_a.sum(0, keepdim=True))
        dW1g.tensor().add_(d_y.t() @ h); db1g.tensor().add_(d_y.sum(0, keepdim=True))
