"""The kernel-interface test double (tests/fake_kernels.py) with the input-gradient entry point, `gcn_input_bwd`: the
specification of twog_gcn_input_bwd (include/twog_gcn.h) stated in torch. It runs in the dtype of its operands, so fp64
operands give the fp64 specification the GPU tests judge the kernel against."""
from tests.fake_kernels import FakeKernels


class InputGradFakeKernels(FakeKernels):
    def gcn_input_bwd(self, x_human, n_nodes, ab, mean_invstd, w1, de1, dgamma, dbeta, training, grad_x_human):
        """grad_x_human[b, t, 0, 2048:] = BatchNorm backward of dx^ = de1 W1 (de1 already ReLU-masked); zeros for the humans
        1 .. H-1. Channel c*N + n sits at memory position n*4 + c."""
        N = n_nodes
        bs, T, H, Fh = x_human.shape

        def pos(v):   # per channel [4N] -> per (node, feature) [N, 4]
            return v.view(4, N).t()

        dxh = (de1 @ w1).view(-1, N, 4)                       # (F, N, 4)
        a = pos(ab[0])
        if training:
            M = dxh.shape[0]                                   # frames behind the batch statistics
            x_n = (self._geo(x_human, N) - pos(mean_invstd[0])) * pos(mean_invstd[1])
            dx = a * (dxh - pos(dbeta) / M - x_n * (pos(dgamma) / M))
        else:
            dx = a * dxh
        grad_x_human[:, :, 0, 2048:] = dx.reshape(bs, T, 4 * N)
        grad_x_human[:, :, 1:, 2048:] = 0
        return grad_x_human
