"""The kernel-interface test double (tests/fake_kernels.py) with `matmul_precision`, the context manager of
HipKernels.matmul_precision: it validates the name like the real one and records ('enter', name) / ('exit', name) in
`precision_events`. `precision_depth` is the nesting depth at the moment (0 outside every context). For the CPU tests of the
host layer in 2g-gcn_amd/ops.py and models.py; the double's arithmetic does not depend on the setting."""
import contextlib

from tests.fake_kernels import FakeKernels


class MatmulPrecisionFakeKernels(FakeKernels):
    MATMUL_PRECISIONS = ('highest', 'high', 'medium')

    def __init__(self):
        super().__init__()
        self.precision_events = []
        self.precision_depth = 0

    @contextlib.contextmanager
    def matmul_precision(self, name):
        if name not in self.MATMUL_PRECISIONS:
            raise ValueError(f'matmul precision must be one of {list(self.MATMUL_PRECISIONS)}, not {name!r}')
        self.precision_events.append(('enter', name))
        self.precision_depth += 1
        try:
            yield
        finally:
            self.precision_depth -= 1
            self.precision_events.append(('exit', name))
