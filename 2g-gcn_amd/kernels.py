"""Tensor-level interface to the gfx950 kernels (lib2ggcn_hip.so).

Every method takes torch CUDA fp32 tensors (or strided views of them), turns them into raw device pointers + strides
and calls ONE C-ABI entry point of include/twog_gcn.h on torch's current HIP stream. torch is used only to own device
memory and streams; no torch math runs here. There is no CPU / eager fallback: on a box without the built library
``HipKernels()`` raises.

Row-strided views: a matrix operand may be a 2-D view (rows, cols) or a 3-D view (outer, inner, cols) with unit
stride on cols -- it maps onto twog_rows_t without a copy.
"""
import contextlib
import ctypes as C
import math
import os

import torch

from . import _lib as L
from .persist import PersistentLaunches

PERSIST = PersistentLaunches()   # admission and failure handling of the persistent launches: the one instance of the process


def _ptr(t):
    return 0 if t is None else t.data_ptr()


_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_CUR_DEVICE = getattr(torch._C, '_cuda_getDevice', None)
if _CUR_DEVICE is None:
    _RAW_STREAM = None


def rows_of(t):
    """twog_rows_t of a 2-D (rows, cols) or 3-D (outer, inner, cols) fp32 view with unit column stride."""
    r = L.Rows()
    if t is None:
        r.ptr, r.ld_outer, r.ld_inner, r.inner = 0, 0, 0, 1
        return r
    assert t.dtype == torch.float32, t.dtype
    assert t.dim() in (2, 3), t.shape
    assert t.shape[-1] == 1 or t.stride(-1) == 1, (t.shape, t.stride())
    r.ptr = t.data_ptr()
    if t.dim() == 2:
        r.inner, r.ld_outer, r.ld_inner = 1, t.stride(0), t.stride(0)
    else:
        r.inner, r.ld_outer, r.ld_inner = t.shape[1], t.stride(0), t.stride(1)
        if t.shape[1] == 1:
            r.inner, r.ld_inner = 1, t.stride(0)
    return r


def fill_rows(r, t):
    """rows_of(t) written into the existing twog_rows_t `r` (a field of a descriptor array: no temporary, no copy)."""
    assert t.dtype == torch.float32, t.dtype
    nd = t.dim()
    st = t.stride()
    assert nd in (2, 3) and (t.shape[-1] == 1 or st[-1] == 1), (t.shape, st)
    r.ptr = t.data_ptr()
    if nd == 2 or t.shape[1] == 1:
        r.inner, r.ld_outer, r.ld_inner = 1, st[0], st[0]
    else:
        r.inner, r.ld_outer, r.ld_inner = t.shape[1], st[0], st[1]


def n_rows(t):
    return t.shape[0] if t.dim() == 2 else t.shape[0] * t.shape[1]


def _as_int64(v):
    """A Python int modulo 2^64 as the signed value with the same 64 bits (torch has no unsigned 64-bit dtype)."""
    v = int(v) & (2 ** 64 - 1)
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _f32(v):
    return C.c_float(float(v)).value   # the value the C ABI (float) receives


def optim_state_block(step, skipped, beta1, beta2, powers=None):
    """twog_optim_state_t (include/twog_gcn.h) at step `step` as a uint8 [64] CPU tensor. powers = (beta1^step, beta2^step) as
    stored by a checkpoint; None rebuilds them the way the device keeps them: `step` fp64 multiplications by the fp32 beta."""
    s = L.OptimState()
    s.step, s.skipped = int(step), int(skipped)
    if powers is None:
        b1, b2, p1, p2 = _f32(beta1), _f32(beta2), 1.0, 1.0
        for _ in range(int(step)):
            p1, p2 = p1 * b1, p2 * b2
        powers = (p1, p2)
    s.beta1_pow, s.beta2_pow = float(powers[0]), float(powers[1])
    s.clip_k, s.decay_mul, s.apply = 1.0, 1.0, 1
    return torch.frombuffer(bytearray(bytes(s)), dtype=torch.uint8).clone()


def read_optim_state(state):
    """The fields of a state block as a dict (ONE device-to-host copy of 64 bytes)."""
    s = L.OptimState.from_buffer_copy(state.cpu().numpy().tobytes())
    return {name: getattr(s, name) for name, _ in L.OptimState._fields_ if name != 'reserved_'}


def optim_hyper(h):
    return L.OptimHyper(h['beta1'], h['beta2'], h['eps'], h['weight_decay'], h.get('grad_scale', 1.0), h.get('ema_decay') or 0.0)


def _check_optim_state(state):
    assert state.dtype == torch.uint8 and state.numel() == C.sizeof(L.OptimState) and state.is_contiguous()
    assert state.data_ptr() % 8 == 0


class _DeferredWord:
    """The error word of a persistent launch on its way to pinned host memory behind the launch: an entry of PERSIST.pending.
    Host slot and event come from a ring per device, so that a training step allocates nothing."""
    _rings = {}   # device index -> ([pinned int32 [1] tensors], [events], next)

    def __init__(self, i, word, what, n=32):
        ring = self._rings.get(i)
        if ring is None:
            pinned = torch.zeros(n, dtype=torch.int32).pin_memory()
            ring = self._rings[i] = [[pinned[k:k + 1] for k in range(n)], [torch.cuda.Event() for _ in range(n)], 0]
        k = ring[2]
        ring[2] = (k + 1) % n
        self.host, self.ev, self.what = ring[0][k], ring[1][k], what
        self.host.copy_(word, non_blocking=True)
        self.ev.record()

    def value(self):
        self.ev.synchronize()
        return int(self.host[0])


class HipKernels:
    """The product backend. `tests/fake_kernels.py` implements the same methods in plain torch for CPU-side tests of
    the host logic; it is never reachable from this package."""

    name = 'hip'

    def __init__(self):
        self.lib = L.load()
        self._ws = {}
        self._tape = None
        self._force_wide = False   # tests only: the wide GCN family also for n_nodes <= twog_gcn_max_nodes()

    # ---------------------------------------------------------------- utilities
    def _stream(self):
        # the raw handle of torch's current stream on the current device: two C calls (~0.3 us) instead of the
        # torch.cuda.current_stream() Stream object (~8 us) -- a host-composed step asks for it thousands of times
        if self._tape is not None:
            # Between tape_begin() and tape_end() only the recordable entry points may be called (they return before they get
            # here): anything else would launch NOW, for the composed steps only, and be missing from every replayed step --
            # and the replay could not know. A programming error, raised where it happens.
            raise RuntimeError('a kernel entry point that cannot be recorded was called while a step is being taped '
                               '(kernels.tape_begin): only gemm (not chain), gru_step_*, relation_*_many and rowops may run there')
        if _RAW_STREAM is not None:
            return _RAW_STREAM(_CUR_DEVICE())
        return torch.cuda.current_stream().cuda_stream

    @staticmethod
    def _check(rc, what):
        if rc != 0:
            raise RuntimeError(f'{what} failed with code {rc}')

    def empty(self, *shape, like=None, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=like.device)

    def zeros(self, *shape, like=None, dtype=torch.float32, device=None):
        """A zeroed buffer: torch owns the memory, the library clears it (twog_fill_zero) -- no ATen kernel on the path."""
        t = torch.empty(*shape, dtype=dtype, device=like.device if like is not None else device)
        return self.fill_zero(t)

    def fill_zero(self, t):
        """In-place clear of a contiguous tensor (the whole storage range it spans)."""
        assert t.is_contiguous()
        if t.numel():
            self._check(self.lib.twog_fill_zero(t.data_ptr(), t.numel() * t.element_size(), self._stream()), 'twog_fill_zero')
        return t

    # ---------------------------------------------------------------- side stream (independent work beside a launch chain)
    class _Side:
        """`with side:` issues launches on a second stream of the device; it starts behind everything the caller's stream
        holds at construction, join() makes the caller's stream wait for it. Tensors allocated inside belong to the side
        stream's pool (torch's allocator handles their reuse); tensors of the caller's stream that the side launches read must
        stay referenced until join() (ops keeps them in the saved state of the pass)."""

        def __init__(self, stream):
            self.main = torch.cuda.current_stream()
            self.stream = stream
            ev = torch.cuda.Event()
            ev.record(self.main)
            stream.wait_event(ev)
            self._ctx = None

        def __enter__(self):
            self._ctx = torch.cuda.stream(self.stream)
            self._ctx.__enter__()
            return self

        def __exit__(self, *a):
            return self._ctx.__exit__(*a)

        def join(self):
            ev = torch.cuda.Event()
            ev.record(self.stream)
            self.main.wait_event(ev)

    _side_streams = {}

    def side_stream(self, dev, cus=0):
        """cus > 0: a stream restricted to that many compute units (twog_stream_create_masked: cus / 8 on each XCD), so that
        what runs on it leaves the other CUs to the caller's stream; None when the runtime refuses the mask. cus = 0: an
        ordinary second stream."""
        key = (self._dev_index(dev), int(cus))
        st = HipKernels._side_streams.get(key)
        if st is None:
            if cus > 0:
                with torch.cuda.device(dev):
                    h = C.c_void_p()
                    rc = self.lib.twog_stream_create_masked(int(cus), C.byref(h))
                st = torch.cuda.ExternalStream(h.value, device=dev) if rc == 0 and h.value else False
            elif os.environ.get('TWOG_SIDE_PRIORITY', 'normal') == 'low':
                # (experiment, round 6: the side stream's GEMM workgroups at the lowest queue priority, so that the chain's
                # workgroups on the caller's stream win free compute units; profiles/r06_side_stream_priority_ab.txt)
                with torch.cuda.device(dev):
                    h = C.c_void_p()
                    rc = self.lib.twog_stream_create_low_priority(C.byref(h))
                st = torch.cuda.ExternalStream(h.value, device=dev) if rc == 0 and h.value else torch.cuda.Stream(device=dev)
            else:
                st = torch.cuda.Stream(device=dev)
            HipKernels._side_streams[key] = st
        return HipKernels._Side(st) if st else None

    # twog_stream_grid: TWOG_STREAM_* of include/twog_gcn.h
    (STREAM_RELU_BWD_VEC, STREAM_RELU_BWD, STREAM_ADD_ROWS, STREAM_RANK1_VEC, STREAM_RANK1, STREAM_ROWOPS, STREAM_ADAM,
     STREAM_MUL, STREAM_SCALE_ROWS, STREAM_COPY_BLOCKS, STREAM_FILL_ZERO, STREAM_REORDER) = range(12)
    STREAM_THREADS = 256   # TWOG_STREAM_THREADS

    def stream_grid(self, kernel, work, cols=0):
        """Workgroups the launcher of the capped grid-stride kernel `kernel` (STREAM_*) uses for `work` items (elements; bytes for
        STREAM_FILL_ZERO); STREAM_REORDER: the column chunks for `work` (clip, entity) pairs of `cols` columns. Host arithmetic of
        the library, no GPU call."""
        g = self.lib.twog_stream_grid(int(kernel), int(work), int(cols))
        if g < 0:
            raise RuntimeError(f'twog_stream_grid failed with code {g}')
        return g

    def debug_occupy(self, n_blocks, lds_bytes, usec):
        """Diagnostics (tests): n_blocks workgroups holding lds_bytes of LDS each for usec microseconds on the current stream."""
        self._check(self.lib.twog_debug_occupy(n_blocks, lds_bytes, usec, self._stream()), 'twog_debug_occupy')

    def copy_blocks(self, pairs):
        """pairs: (src, dst) contiguous fp32 tensors of equal element count; dst[...] = src[...] for all of them in ONE
        launch (twog_copy_blocks) -- the per-forward build of the packed operands (ops.pack_weights)."""
        pairs = [(s, d) for s, d in pairs if s.numel()]
        for i in range(0, len(pairs), L.COPY_MAX):
            chunk = pairs[i:i + L.COPY_MAX]
            arr = (L.Copy * len(chunk))()
            for a, (s, d) in zip(arr, chunk):
                assert s.dtype == torch.float32 and d.dtype == torch.float32 and s.is_contiguous() and d.is_contiguous()
                assert s.numel() == d.numel() and s.device == d.device
                a.src, a.dst, a.n = s.data_ptr(), d.data_ptr(), s.numel()
            self._check(self.lib.twog_copy_blocks(arr, len(chunk), self._stream()), 'twog_copy_blocks')

    def zeros_many(self, shapes, device, dtype=torch.float32):
        """Zeroed fp32 buffers of the given shapes carved out of ONE allocation and cleared by ONE launch (each view starts
        on a 256-byte boundary)."""
        sizes = [int(math.prod(sh)) for sh in shapes]
        offs, total = [], 0
        for n in sizes:
            offs.append(total)
            total += (n + 63) // 64 * 64
        buf = self.zeros(max(total, 1), dtype=dtype, device=device)
        return [buf[o:o + n].view(*sh) for o, n, sh in zip(offs, sizes, shapes)]

    def workspace(self, nbytes, device, key='ws'):
        """A persistent scratch buffer per (device, key, current stream); grown on demand, contents undefined between
        calls. Per stream because launches on different streams may run concurrently (split-K slabs, reduction partials);
        launches that share a buffer are ordered by their stream."""
        k = (str(device), key, int(self._stream() or 0))
        buf = self._ws.get(k)
        if buf is None or buf.numel() * 4 < nbytes:
            buf = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
            if key == 'splitk':
                # the first 16 KB of the split-K workspace are reserved and handed over zeroed, as twog_gemm_f32 asks
                # (include/twog_gcn.h); the slabs start behind them
                self.fill_zero(buf[:4096])
            self._ws_put(k, buf)
        else:
            self._ws_touch(k)
        return buf

    MAX_STREAMS_PER_WORKSPACE = 4

    def _ws_touch(self, k):
        self._ws[k] = self._ws.pop(k)   # most recently used last (dict order)

    def _ws_put(self, k, buf):
        """Workspaces are per (device, kind, stream): at most MAX_STREAMS_PER_WORKSPACE streams keep one of each kind, the
        least recently used entry goes first (a 320 MB split-K buffer + a 48 MB chain workspace per stream that ever
        issued a GEMM would otherwise stay for the life of the process). Dropping an entry only drops torch's reference:
        the caching allocator keeps the memory valid for work already enqueued on the stream that used it."""
        self._ws.pop(k, None)
        self._ws[k] = buf
        same = [q for q in self._ws if q[0] == k[0] and q[1] == k[1]]
        for q in same[:-self.MAX_STREAMS_PER_WORKSPACE]:
            del self._ws[q]

    def release_workspaces(self):
        """Drops every cached workspace (they are re-created on demand)."""
        self._ws.clear()

    def chain_workspace(self, device):
        """(pointer, bytes) of the chain workspace of the CURRENT stream on `device` (include/twog_gcn.h,
        twog_gemm_f32_chain): arrival tickets (zeroed here, once; every launch returns them to zero) + room for the
        partial tiles of a reduction split over workgroups. One buffer per (device, stream): launches that share it are
        ordered by the stream."""
        k = (str(device), 'chain', int(self._stream() or 0))
        buf = self._ws.get(k)
        if buf is None:
            buf = torch.zeros(int(self.lib.twog_chain_workspace_bytes()) // 4, dtype=torch.float32, device=device)
            self._ws_put(k, buf)
        return buf.data_ptr(), buf.numel() * 4

    def version(self):
        return self.lib.twog_version().decode()

    # ---------------------------------------------------------------- GEMM
    def _gemm_array(self, problems, a_kmajor, b_kmajor):
        n = len(problems)
        arr = (L.Gemm * n)()
        for i, p in enumerate(problems):
            A, B, Cm = p['A'], p['B'], p['C']
            g = arr[i]
            fill_rows(g.A, A)
            fill_rows(g.B, B)
            fill_rows(g.C, Cm)
            if a_kmajor:
                K, M = n_rows(A), A.shape[-1]
            else:
                M, K = n_rows(A), A.shape[-1]
            if b_kmajor:
                Kb, N = n_rows(B), B.shape[-1]
            else:
                N, Kb = n_rows(B), B.shape[-1]
            assert K == Kb, (A.shape, B.shape, a_kmajor, b_kmajor)
            assert n_rows(Cm) == M and Cm.shape[-1] == N, (Cm.shape, M, N)
            bias = p.get('bias')
            if bias is not None:
                assert bias.numel() == N and bias.is_contiguous()
            g.bias = _ptr(bias)
            g.M, g.N, g.K = M, N, K
            g.act = int(p.get('act', 0))
            g.accumulate = int(bool(p.get('accumulate', False)))
            b = p.get('batch')
            if b is None:
                g.batch, g.a_batch_stride, g.b_batch_stride, g.c_batch_stride = 1, 0, 0, 0
            else:
                g.batch, g.a_batch_stride, g.b_batch_stride, g.c_batch_stride = b
            cs = p.get('colsum')
            if cs is not None:
                assert a_kmajor and cs.numel() == M and cs.is_contiguous() and cs.dtype == torch.float32
            g.a_colsum = _ptr(cs)
            g.a_colsum_accumulate = int(bool(p.get('colsum_accumulate', False)))
        return arr

    def gemm_colsum_ok(self, problem):
        """True if gemm([problem], a_kmajor=True, b_kmajor=True) with a 'colsum' entry takes the column sums of A inside the
        GEMM launch (twog_gemm_colsum_fused); False: the caller takes them with colsum()."""
        key = tuple((tuple(t.shape), tuple(t.stride()), t.data_ptr() % 16) for t in (problem['A'], problem['B'], problem['C']))
        ok = self._colsum_ok.get(key)
        if ok is None:
            arr = self._gemm_array([dict(problem, colsum=None)], True, True)
            arr[0].a_colsum = arr[0].C.ptr   # (any non-null pointer: the query launches nothing)
            ws = self.workspace(320 << 20, problem['C'].device, 'splitk')
            ok = self._colsum_ok[key] = bool(self.lib.twog_gemm_colsum_fused(arr, 1, 1, 1, ws.data_ptr(), ws.numel() * 4))
        return ok

    _colsum_ok = {}

    def gemm(self, problems, a_kmajor=False, b_kmajor=False, split_k_workspace=True, chain=False):
        """problems: list of dicts with keys A, B, C (row-strided views), bias (1-D or None), act (0/1), accumulate.
        Logical shapes: A (M,K) [or stored (K,M) if a_kmajor], B (N,K) [or (K,N) if b_kmajor], C (M,N).
        Optional 'batch': (n, a_stride, b_stride, c_stride) in elements. chain=True: a launch of a recurrent chain
        (twog_gemm_f32_chain: the reduction may be split over workgroups and combined inside the launch).
        Optional 'colsum' ([M] fp32, with 'colsum_accumulate'): the column sums of a k-major A from the same pass over A
        (twog_gemm_t::a_colsum; only where gemm_colsum_ok(problem) holds)."""
        n = len(problems)
        if n == 0:
            return
        dev = problems[0]['C'].device
        arr = self._gemm_array(problems, a_kmajor, b_kmajor)
        if chain:
            assert self._tape is None, 'chain launches cannot be recorded (kernels.tape_begin)'
            rc = self.lib.twog_gemm_f32_chain(arr, n, int(a_kmajor), int(b_kmajor), *self.chain_workspace(dev), self._stream())
            self._check(rc, 'twog_gemm_f32_chain')
            return
        if self._tape is not None:
            self._tape.append((L.TAPE_GEMM, n, int(a_kmajor) | int(b_kmajor) << 1, arr))
            return
        ws_ptr, ws_bytes = 0, 0
        if split_k_workspace:
            ws = self.workspace(320 << 20, dev, 'splitk')
            ws_ptr, ws_bytes = ws.data_ptr(), ws.numel() * 4
        rc = self.lib.twog_gemm_f32(arr, n, int(a_kmajor), int(b_kmajor), ws_ptr, ws_bytes, self._stream())
        self._check(rc, 'twog_gemm_f32')

    GEMM_TILE128, GEMM_WAVES8, GEMM_KG, GEMM_SPLITK, GEMM_GATE, GEMM_KSPLIT, GEMM_GRUFWD, GEMM_ROWS32 = 1, 2, 4, 8, 16, 32, 64, 128  # TWOG_GEMM_CLASS_*
    GEMM_XSPLIT = 256
    GEMM_X3 = 512
    GEMM_P3, GEMM_P1 = 1024, 2048   # beside GEMM_X3 on the 128x128 class: the 'high' (3 products) / 'medium' (1 product) kernels ran

    def gemm_last_class(self):
        """Bit field (GEMM_*) of the kernel variant the most recent gemm() chunk of this thread selected."""
        return int(self.lib.twog_gemm_last_class())

    MATMUL_PRECISIONS = {'highest': 0, 'high': 1, 'medium': 2}   # TWOG_GEMM_PRECISION_*

    @contextlib.contextmanager
    def matmul_precision(self, name):
        """The GEMMs of the bf16x3 128x128 class that THIS thread launches inside the block keep six ('highest', the default),
        three ('high') or one ('medium') chunk product per multiply (twog_gemm_set_precision); every other kernel is unaffected.
        The previous setting comes back on exit, also when the block raises."""
        if name not in self.MATMUL_PRECISIONS:
            raise ValueError(f"matmul precision must be one of {sorted(self.MATMUL_PRECISIONS)}, not {name!r}")
        prev = int(self.lib.twog_gemm_set_precision(self.MATMUL_PRECISIONS[name]))
        try:
            yield
        finally:
            self.lib.twog_gemm_set_precision(prev)

    # ---------------------------------------------------------------- geometric-level GCN
    @staticmethod
    def _geo(x_human):
        """x_human (bs, T, H, 2048+4N) contiguous -> (pointer to geometry of human 0 of frame 0, frame stride, frames)."""
        assert x_human.is_contiguous() and x_human.dtype == torch.float32
        bs, T, H, Fh = x_human.shape
        return x_human.data_ptr() + 2048 * 4, H * Fh, bs * T

    # twog_gcn_launch_plan: TWOG_GCN_PLAN_* of include/twog_gcn.h
    PLAN_FUSED_FWD, PLAN_ATTN2_FWD, PLAN_ATTN2_BWD, PLAN_EMBED1_FWD, PLAN_ATTN_FWD, PLAN_ATTN_BWD = range(6)

    def gcn_launch_plan(self, kernel, n_frames, n_nodes):
        """(grid, frames per group, dynamic LDS bytes, variant) the launcher of `kernel` (PLAN_*) uses at this size; host
        arithmetic of the library, no GPU call. variant: NT of the fused forward kernel, with_m of gcn_attn2_bwd."""
        out = (C.c_int * 4)()
        self._check(self.lib.twog_gcn_launch_plan(kernel, n_frames, n_nodes, out), 'twog_gcn_launch_plan')
        return tuple(out)

    # twog_gcn_wide_launch_plan: TWOG_GCN_WIDE_PLAN_* of include/twog_gcn.h
    WIDE_PLAN_FWD, WIDE_PLAN_BWD, WIDE_PLAN_EMBED1_FWD = range(3)

    def gcn_wide_launch_plan(self, kernel, n_frames, n_nodes):
        """gcn_launch_plan of the wide family (n_nodes <= twog_gcn_wide_max_nodes()): (grid, frames per trip, dynamic LDS bytes,
        variant) for `kernel` (WIDE_PLAN_*); host arithmetic of the library, no GPU call."""
        out = (C.c_int * 4)()
        self._check(self.lib.twog_gcn_wide_launch_plan(kernel, n_frames, n_nodes, out), 'twog_gcn_wide_launch_plan')
        return tuple(out)

    def _gcn_wide(self, n_nodes):
        """Which kernel family the six geometric-level GCN methods below call: the tuned kernels up to twog_gcn_max_nodes(), the
        wide family (csrc/geo_wide.hip) beyond. The only place where the choice is made."""
        return self._force_wide or n_nodes > self.lib.twog_gcn_max_nodes()

    def _gcn_entry(self, name, n_nodes):
        """(entry point, its name) of the tuned kernel `name` or of its twog_gcn_wide_* twin."""
        if self._gcn_wide(n_nodes):
            name = self._WIDE_TWIN[name]
        return getattr(self.lib, name), name

    _WIDE_TWIN = {'twog_bn_stats': 'twog_gcn_wide_bn_stats', 'twog_bn_finalize': 'twog_gcn_wide_bn_finalize',
                  'twog_gcn_embed1_fwd': 'twog_gcn_wide_embed1_fwd', 'twog_gcn_fused_fwd': 'twog_gcn_wide_fwd',
                  'twog_gcn_attn2_bwd': 'twog_gcn_wide_bwd', 'twog_gcn_embed1_bwd': 'twog_gcn_wide_embed1_bwd',
                  'twog_gcn_input_bwd': 'twog_gcn_wide_input_bwd'}

    @staticmethod
    def bn_stats_blocks(n_frames):
        """Workgroups of twog_bn_stats: >= 8 frames per block, at most 240 blocks (the finalize kernel sums them 4-wide)."""
        return max(1, min(240, n_frames // 8))

    @staticmethod
    def embed1_bwd_blocks(n_rows):
        """Workgroups (= partial rows) of twog_gcn_embed1_bwd: 4 waves per block, >= 8 rows per wave."""
        return max(1, min(2048, (n_rows + 31) // 32))

    def bn_fold(self, x_human, n_nodes, gamma, beta, running_mean, running_var, num_batches_tracked, training,
                stats_reduce=None, fold=None):
        """stats_reduce (optional, sync-BN of distributed.DataParallel): callable (sums fp64 [2*4N], n_frames) ->
        (sums reduced over the ranks, total frames); applied to the batch statistics before they are folded.
        fold = (wq [128,64], wk [128,64], bq [128]): the same launch also folds the similarity projections into
        md [65,64] = [Mt | d] (see twog_bn_finalize); then returns (ab, mi, md)."""
        ptr, fstride, nf = self._geo(x_human)
        nch = 4 * n_nodes
        dev = x_human.device
        ab = torch.empty(2, nch, dtype=torch.float32, device=dev)
        mi = torch.empty(2, nch, dtype=torch.float32, device=dev)
        nblk = self.bn_stats_blocks(nf)
        partials = torch.empty(nblk * 2 * nch, dtype=torch.float64, device=dev)
        if training:
            fn, what = self._gcn_entry('twog_bn_stats', n_nodes)
            self._check(fn(ptr, fstride, nf, n_nodes, partials.data_ptr(), nblk, self._stream()), what)
            if stats_reduce is not None:
                partials, nf = stats_reduce(partials.view(nblk, 2 * nch).sum(0), nf)
                partials, nblk = partials.contiguous(), 1
        md = torch.empty(65, 64, dtype=torch.float32, device=dev) if fold is not None else None
        wq, wk, bq = fold if fold is not None else (None, None, None)
        fn, what = self._gcn_entry('twog_bn_finalize', n_nodes)
        self._check(fn(partials.data_ptr(), nblk, nf, n_nodes, gamma.data_ptr(), beta.data_ptr(), running_mean.data_ptr(),
                       running_var.data_ptr(), _ptr(num_batches_tracked), int(training), ab.data_ptr(), mi.data_ptr(),
                       _ptr(wq), _ptr(wk), _ptr(bq), _ptr(md), self._stream()), what)
        return (ab, mi) if fold is None else (ab, mi, md)

    def gcn_embed1_fwd(self, x_human, n_nodes, ab, w1, b1):
        ptr, fstride, nf = self._geo(x_human)
        e1 = torch.empty(nf * n_nodes, 64, dtype=torch.float32, device=x_human.device)
        fn, what = self._gcn_entry('twog_gcn_embed1_fwd', n_nodes)
        self._check(fn(ptr, fstride, nf, n_nodes, ab.data_ptr(), w1.data_ptr(), b1.data_ptr(), e1.data_ptr(), self._stream()),
                    what)
        return e1

    def gcn_fused_fwd(self, x_human, n_nodes, ab, w1, b1, w2, b2, md, save_x=True):
        """Geo_gcn forward up to the aggregation in one kernel: returns (X or None, adj [F,N,N], Z [(f,n),64])."""
        ptr, fstride, nf = self._geo(x_human)
        dev = x_human.device
        X = torch.empty(nf * n_nodes, 64, dtype=torch.float32, device=dev) if save_x else None
        adj = torch.empty(nf, n_nodes, n_nodes, dtype=torch.float32, device=dev)
        Z = torch.empty(nf * n_nodes, 64, dtype=torch.float32, device=dev)
        fn, what = self._gcn_entry('twog_gcn_fused_fwd', n_nodes)
        self._check(fn(ptr, fstride, nf, n_nodes, ab.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                       md.data_ptr(), _ptr(X), adj.data_ptr(), Z.data_ptr(), self._stream()), what)
        return X, adj, Z

    def gcn_embed1_bwd(self, x_human, n_nodes, ab, mean_invstd, w1, de1):
        ptr, fstride, nf = self._geo(x_human)
        dev = x_human.device
        nblk = self.embed1_bwd_blocks(nf * n_nodes)
        partials = torch.empty(nblk * (320 + 8 * n_nodes), dtype=torch.float32, device=dev)
        dw1 = torch.empty(64, 4, dtype=torch.float32, device=dev)
        db1 = torch.empty(64, dtype=torch.float32, device=dev)
        dgamma = torch.empty(4 * n_nodes, dtype=torch.float32, device=dev)
        dbeta = torch.empty(4 * n_nodes, dtype=torch.float32, device=dev)
        fn, what = self._gcn_entry('twog_gcn_embed1_bwd', n_nodes)
        self._check(fn(ptr, fstride, nf, n_nodes, ab.data_ptr(), mean_invstd.data_ptr(), w1.data_ptr(), de1.data_ptr(),
                       partials.data_ptr(), nblk, dw1.data_ptr(), db1.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                       self._stream()), what)
        return dw1, db1, dgamma, dbeta

    @staticmethod
    def input_bwd_blocks(n_rows):
        """Workgroups of twog_gcn_input_bwd: 64 (frame, node) rows per workgroup and trip, at most 2048 workgroups."""
        return max(1, min(2048, (n_rows + 63) // 64))

    def gcn_input_bwd(self, x_human, n_nodes, ab, mean_invstd, w1, de1, dgamma, dbeta, training, grad_x_human):
        """Writes the geometry columns of grad_x_human (same shape as x_human, contiguous): d loss / d x_human[b, t, 0, 2048:]
        from the ReLU-masked de1, zeros for the other humans. Train mode needs the dgamma / dbeta of gcn_embed1_bwd (issued
        before, on the same stream); eval mode takes None for them."""
        ptr, fstride, nf = self._geo(x_human)
        gptr, gstride, _ = self._geo(grad_x_human)
        assert grad_x_human.shape == x_human.shape and gstride == fstride
        bs, T, H, Fh = x_human.shape
        assert Fh == 2048 + 4 * n_nodes and de1.is_contiguous() and w1.is_contiguous()
        fn, what = self._gcn_entry('twog_gcn_input_bwd', n_nodes)
        self._check(fn(ptr, fstride, nf, n_nodes, H, Fh, ab.data_ptr(), _ptr(mean_invstd), w1.data_ptr(), de1.data_ptr(),
                       _ptr(dgamma), _ptr(dbeta), int(bool(training)), gptr, self.input_bwd_blocks(nf * n_nodes),
                       self._stream()), what)
        return grad_x_human

    def gcn_attn_fwd(self, qk, x, n_frames, n_nodes):
        s = torch.empty(n_frames, n_nodes, n_nodes, dtype=torch.float32, device=qk.device)
        z = torch.empty(n_frames * n_nodes, 64, dtype=torch.float32, device=qk.device)
        self._check(self.lib.twog_gcn_attn_fwd(qk.data_ptr(), x.data_ptr(), n_frames, n_nodes, s.data_ptr(),
                                               z.data_ptr(), self._stream()), 'twog_gcn_attn_fwd')
        return s, z

    def gcn_attn2_fwd(self, x, md, n_frames, n_nodes):
        """Folded-projection adjacency attention on MFMA: returns (adj [nF,N,N], z [nF*N,64])."""
        s = torch.empty(n_frames, n_nodes, n_nodes, dtype=torch.float32, device=x.device)
        z = torch.empty(n_frames * n_nodes, 64, dtype=torch.float32, device=x.device)
        self._check(self.lib.twog_gcn_attn2_fwd(x.data_ptr(), md.data_ptr(), n_frames, n_nodes, s.data_ptr(),
                                                z.data_ptr(), self._stream()), 'twog_gcn_attn2_fwd')
        return s, z

    def gcn_attn2_bwd(self, x, md, s, dz, n_frames, n_nodes):
        """Returns (dx_att [nF*N,64], dmd [65,64] = gradient wrt (Mt | d))."""
        dx = torch.empty(n_frames * n_nodes, 64, dtype=torch.float32, device=x.device)
        if self._gcn_wide(n_nodes):
            nblk = self.gcn_wide_launch_plan(self.WIDE_PLAN_BWD, n_frames, n_nodes)[0]
        else:
            nblk = self.lib.twog_gcn_attn2_bwd_blocks(n_frames)
        partials = torch.empty(nblk, 65 * 64, dtype=torch.float32, device=x.device)
        fn, what = self._gcn_entry('twog_gcn_attn2_bwd', n_nodes)
        self._check(fn(x.data_ptr(), md.data_ptr(), s.data_ptr(), dz.data_ptr(), n_frames, n_nodes, dx.data_ptr(),
                       partials.data_ptr(), nblk, self._stream()), what)
        return dx, self.colsum(partials).view(65, 64)

    def gcn_attn_bwd(self, qk, x, s, dz, n_frames, n_nodes):
        dx = torch.empty(n_frames * n_nodes, 64, dtype=torch.float32, device=qk.device)
        dqk = torch.empty(n_frames * n_nodes, 256, dtype=torch.float32, device=qk.device)
        self._check(self.lib.twog_gcn_attn_bwd(qk.data_ptr(), x.data_ptr(), s.data_ptr(), dz.data_ptr(), n_frames,
                                               n_nodes, dx.data_ptr(), dqk.data_ptr(), self._stream()),
                    'twog_gcn_attn_bwd')
        return dx, dqk

    # ---------------------------------------------------------------- frame-level BiGRU
    def bigru_fwd(self, types, bs, T, h):
        """types: list of dicts {gi (bs,T,E,6h), w_hh_f, b_hh_f, w_hh_r, b_hh_r}. Returns [(out (bs,T,E,2h), save)]."""
        n = len(types)
        arr = (L.BiGru * n)()
        outs, keep = [], []
        for i, y in enumerate(types):
            gi = y['gi']
            E = gi.shape[2]
            dev = gi.device
            assert gi.is_contiguous() and gi.shape == (bs, T, E, 6 * h)
            out = torch.empty(bs, T, E, 2 * h, dtype=torch.float32, device=dev)
            save = torch.empty(2, bs, T, E, 4 * h, dtype=torch.float32, device=dev)
            tmp = torch.empty(2, bs * E, 3 * h, dtype=torch.float32, device=dev)
            zeros = self.zeros(bs * E, h, device=dev)
            keep += [tmp, zeros]
            a = arr[i]
            a.gi, a.w_hh_f, a.b_hh_f, a.w_hh_r, a.b_hh_r = (gi.data_ptr(), y['w_hh_f'].data_ptr(),
                                                             _ptr(y.get('b_hh_f')), y['w_hh_r'].data_ptr(),
                                                             _ptr(y.get('b_hh_r')))
            a.out, a.save, a.tmp_gh, a.zeros, a.E = out.data_ptr(), save.data_ptr(), tmp.data_ptr(), zeros.data_ptr(), E
            outs.append((out, save))
        mode = os.environ.get('TWOG_BIGRU_PERSIST', 'auto')
        # small batches: one persistent launch, W_hh slices resident in LDS (csrc/gru_persist.hip); =1: wherever it is served
        self.last_bigru_persistent = self._try_persistent(
            'bigru_fwd', dev, mode, lambda: self.lib.twog_bigru_persistent_supported(arr, n, bs, h),
            lambda sync: self.lib.twog_bigru_fwd_persistent(arr, n, bs, T, h, sync, self._stream()),
            n_sync=1024, err_index=128, threshold=1 if mode == '1' else 2)
        if not self.last_bigru_persistent:
            self._check(self.lib.twog_bigru_fwd(arr, n, bs, T, h, *self.chain_workspace(dev), self._stream()), 'twog_bigru_fwd')
        return outs

    # ---- the persistent launches: policy and state in persist.py (PERSIST); here the launches and the device side of the checks
    @staticmethod
    def _dev_index(dev=None):
        return dev.index if dev is not None and dev.index is not None else torch.cuda.current_device()

    def persistent_allowed(self, launch, dev):
        """PERSIST.allowed for the launch 'bigru_fwd' | 'bigru_bwd' | 'segrnn_fwd' | 'segrnn_bwd' on its device."""
        return PERSIST.allowed(self._dev_index(dev))

    def _persistent_admitted(self, launch, dev, mode, rating, threshold=2, key=None, allow=True):
        """The admission decision of every persistent launch, in the one order that matters: the launch's environment switch
        (mode), the caller's veto, the memo of refused grids, the library's rating() of the shape (0 not served, 1 served, 2
        also the faster path) and LAST persistent_allowed: it consumes a back-off credit, which only a launch that would
        otherwise be attempted may do."""
        return (mode != '0' and allow and key not in PERSIST.refused and int(rating()) >= threshold
                and self.persistent_allowed(launch, dev))

    def _try_persistent(self, launch, dev, mode, rating, run, n_sync, err_index, threshold=2, key=None, allow=True):
        """Decide, attempt, else fall through, for all four launches (csrc/gru_persist.hip, seg_persist.hip). True: the
        persistent launch served the pass. False (not admitted, not resident, or a wait ran out): the caller runs the
        launch-per-step path, on the same buffers. run(sync pointer) launches on n_sync sync words, zeroed per call, and returns
        the return code; the launch's error word is word err_index of them."""
        if not self._persistent_admitted(launch, dev, mode, rating, threshold, key, allow):
            return False
        sync = self.zeros(n_sync, device=dev)
        rc = run(sync.data_ptr())
        i, what, word = self._dev_index(dev), f'twog_{launch}_persistent', sync.view(torch.int32)[err_index:err_index + 1]
        return PERSIST.completed(i, rc, what, lambda: int(word.item()), lambda: _DeferredWord(i, word, what), key)

    def verify_persistent(self, dev=None):
        """End of a forward / backward pass: every persistent launch of the pass whose error word was left for later must
        have completed. Raises RuntimeError otherwise (persist.py)."""
        PERSIST.verify(self._dev_index(dev))

    def guard_persistent(self, dev, outs):
        """End of a forward pass that a backward pass will follow: instead of waiting for the pass's deferred error words
        (verify_persistent drains the stream, and the backward pass is then enqueued into an idle device: ~1 ms per 8-clip
        step), ONE small launch behind them overwrites `outs` with NaN if any is set. The words stay pending: the check at
        the end of the backward pass (or at the start of the next forward) raises. True when nothing is pending or the guard
        was enqueued; False -> the caller verifies at once."""
        pending = PERSIST.pending.get(self._dev_index(dev))
        if not pending:
            return True
        outs = [o for o in outs if o is not None and o.numel()]
        if (len(pending) > L.GUARD_MAX or len(outs) > L.GUARD_MAX or os.environ.get('TWOG_PERSIST_GUARD', '1') == '0'
                or any(o.dtype != torch.float32 or not o.is_contiguous() for o in outs)):
            return False
        g = L.Guard()
        for k, d in enumerate(pending):
            g.words[k] = d.host.data_ptr()
        for k, o in enumerate(outs):
            g.out[k], g.n[k] = o.data_ptr(), o.numel()
        g.n_words, g.n_out = len(pending), len(outs)
        self._check(self.lib.twog_guard_outputs(C.byref(g), self._stream()), 'twog_guard_outputs')
        return True

    def bigru_persistent_plan(self, Es, bs, h, n_cus=0):
        """What bigru_fwd / bigru_bwd would launch persistently for entity counts Es at this batch and width on n_cus compute
        units (0: the current device's): forward instance (nkb, twc), grid, LDS bytes, whether the backward is served, and
        the combinations (group, rt0, rt1, tw). Host arithmetic of the library (twog_bigru_persistent_plan), nothing launched."""
        return L.bigru_persistent_plan(self.lib, Es, bs, h, n_cus)

    def bigru_persistent(self, arr, n, bs, h, dev=None):
        """True when the frame-level recurrence runs as the persistent launch: where the library serves the shape and
        rates it the faster path (small batches: at most one 16-row tile per wave). TWOG_BIGRU_PERSIST=1: wherever it is
        served; =0: never."""
        mode = os.environ.get('TWOG_BIGRU_PERSIST', 'auto')
        return self._persistent_admitted('bigru_fwd', dev, mode, lambda: self.lib.twog_bigru_persistent_supported(arr, n, bs, h),
                                         threshold=1 if mode == '1' else 2)

    @staticmethod
    def _bigru_bwd_key(i, Es, bs, h):
        """What PERSIST.refused remembers a refused backward BiGRU grid by (the only launch with a memo: DESIGN.md 7)."""
        return ('bigru_bwd', i, tuple(int(E) for E in Es), bs, h)

    def bigru_bwd_would_persist(self, Es, bs, h):
        """Whether bigru_bwd takes the persistent launch for entity counts Es at this batch (asked before the operands exist:
        the data-parallel backward pass orders its first gradient all-reduce and its side stream around that launch, ADVICE
        r05). What turns the launch down -- a shared device, the back-off window, a grid refused before on this device --
        is read here, not consumed: persistent_allowed() counts the window down when the launch is really attempted."""
        i = self._dev_index()
        if os.environ.get('TWOG_BIGRU_PERSIST', 'auto') == '0' or PERSIST.blocked(i, self._bigru_bwd_key(i, Es, bs, h)):
            return False
        arr = (L.BiGruBwd * len(Es))()
        for a, E in zip(arr, Es):
            a.E = E
        return int(self.lib.twog_bigru_bwd_persistent_supported(arr, len(Es), bs, h)) >= 2

    def bigru_bwd(self, types, bs, T, h, allow_persistent=True):
        """types: list of dicts {d_out, save, out, w_hh_f, w_hh_r}. Returns [(d_gi, d_gh)] each (bs,T,E,6h)."""
        n = len(types)
        arr = (L.BiGruBwd * n)()
        outs, keep = [], []
        for i, y in enumerate(types):
            d_out = y['d_out']
            E = d_out.shape[2]
            dev = d_out.device
            assert d_out.is_contiguous() and d_out.shape == (bs, T, E, 2 * h)
            d_gi = torch.empty(bs, T, E, 6 * h, dtype=torch.float32, device=dev)
            d_gh = torch.empty(bs, T, E, 6 * h, dtype=torch.float32, device=dev)
            carry = torch.empty(2, bs * E, h, dtype=torch.float32, device=dev)
            keep.append(carry)
            a = arr[i]
            a.d_out, a.save, a.out = d_out.data_ptr(), y['save'].data_ptr(), y['out'].data_ptr()
            a.w_hh_f, a.w_hh_r = y['w_hh_f'].data_ptr(), y['w_hh_r'].data_ptr()
            a.d_gi, a.d_gh, a.carry, a.E = d_gi.data_ptr(), d_gh.data_ptr(), carry.data_ptr(), E
            outs.append((d_gi, d_gh))
        self.last_bigru_bwd_persistent = self._try_persistent(   # small batches: one persistent launch (csrc/gru_persist.hip)
            'bigru_bwd', dev, os.environ.get('TWOG_BIGRU_PERSIST', 'auto'),
            lambda: self.lib.twog_bigru_bwd_persistent_supported(arr, n, bs, h),
            lambda sync: self.lib.twog_bigru_bwd_persistent(arr, n, bs, T, h, sync, self._stream()),
            n_sync=1024, err_index=128, allow=allow_persistent,
            key=self._bigru_bwd_key(self._dev_index(dev), (y['d_out'].shape[2] for y in types), bs, h))
        if not self.last_bigru_bwd_persistent:
            self._check(self.lib.twog_bigru_bwd(arr, n, bs, T, h, *self.chain_workspace(dev), self._stream()), 'twog_bigru_bwd')
        return outs

    # ---------------------------------------------------------------- single-direction frame GRU (baseline models)
    def gru_seq_fwd(self, types, bs, T, h):
        """types: list of dicts {gi (bs,T,E,3h), w_hh, b_hh (or None)}. Returns [(out (bs,T,E,h), save (bs,T,E,4h))].
        The forward direction of bigru_fwd alone (twog_gru_seq_fwd); there is no persistent form."""
        n = len(types)
        arr = (L.BiGru * n)()
        outs, keep = [], []
        for i, y in enumerate(types):
            gi = y['gi']
            E = gi.shape[2]
            dev = gi.device
            assert gi.is_contiguous() and gi.shape == (bs, T, E, 3 * h)
            out = torch.empty(bs, T, E, h, dtype=torch.float32, device=dev)
            save = torch.empty(bs, T, E, 4 * h, dtype=torch.float32, device=dev)
            tmp = torch.empty(bs * E, 3 * h, dtype=torch.float32, device=dev)
            zeros = self.zeros(bs * E, h, device=dev)
            keep += [tmp, zeros]
            a = arr[i]
            a.gi, a.w_hh_f, a.b_hh_f, a.w_hh_r, a.b_hh_r = gi.data_ptr(), y['w_hh'].data_ptr(), _ptr(y.get('b_hh')), 0, 0
            a.out, a.save, a.tmp_gh, a.zeros, a.E = out.data_ptr(), save.data_ptr(), tmp.data_ptr(), zeros.data_ptr(), E
            outs.append((out, save))
        self._check(self.lib.twog_gru_seq_fwd(arr, n, bs, T, h, *self.chain_workspace(dev), self._stream()), 'twog_gru_seq_fwd')
        return outs

    def gru_seq_bwd(self, types, bs, T, h):
        """types: list of dicts {d_out (bs,T,E,h), save, out, w_hh}. Returns [(d_gi, d_gh)] each (bs,T,E,3h)."""
        n = len(types)
        arr = (L.BiGruBwd * n)()
        outs, keep = [], []
        for i, y in enumerate(types):
            d_out = y['d_out']
            E = d_out.shape[2]
            dev = d_out.device
            assert d_out.is_contiguous() and d_out.shape == (bs, T, E, h)
            d_gi = torch.empty(bs, T, E, 3 * h, dtype=torch.float32, device=dev)
            d_gh = torch.empty(bs, T, E, 3 * h, dtype=torch.float32, device=dev)
            carry = torch.empty(bs * E, h, dtype=torch.float32, device=dev)
            keep.append(carry)
            a = arr[i]
            a.d_out, a.save, a.out = d_out.data_ptr(), y['save'].data_ptr(), y['out'].data_ptr()
            a.w_hh_f, a.w_hh_r = y['w_hh'].data_ptr(), 0
            a.d_gi, a.d_gh, a.carry, a.E = d_gi.data_ptr(), d_gh.data_ptr(), carry.data_ptr(), E
            outs.append((d_gi, d_gh))
        self._check(self.lib.twog_gru_seq_bwd(arr, n, bs, T, h, *self.chain_workspace(dev), self._stream()), 'twog_gru_seq_bwd')
        return outs

    # ---------------------------------------------------------------- entity pool + concat (baseline models)
    def entity_pool_fwd(self, hfr, ofr, mask, object_head):
        """hfr (bs,T,H,W), ofr (bs,T,O,W), mask (bs,O) -> hin (bs,T,H,2W) = [hfr | masked mean of ofr], and with
        object_head oin (bs,T,O,2W) = [ofr | sum of hfr] (else None)."""
        bs, T, H, W = hfr.shape
        O = ofr.shape[2]
        assert hfr.is_contiguous() and ofr.is_contiguous() and mask.is_contiguous() and mask.dtype == torch.float32
        assert ofr.shape == (bs, T, O, W) and mask.shape == (bs, O)
        hin = torch.empty(bs, T, H, 2 * W, dtype=torch.float32, device=hfr.device)
        oin = torch.empty(bs, T, O, 2 * W, dtype=torch.float32, device=hfr.device) if object_head else None
        d = L.EntityPool()
        d.hfr, d.ofr, d.mask, d.hin, d.oin = hfr.data_ptr(), ofr.data_ptr(), mask.data_ptr(), hin.data_ptr(), _ptr(oin)
        d.bs, d.T, d.H, d.O, d.W = bs, T, H, O, W
        self._check(self.lib.twog_entity_pool_fwd(C.byref(d), self._stream()), 'twog_entity_pool_fwd')
        return hin, oin

    def entity_pool_bwd(self, d_hin, d_oin, mask, O):
        """Gradients of entity_pool_fwd: returns (d_hfr (bs,T,H,W), d_ofr (bs,T,O,W)). d_oin None: no object head."""
        bs, T, H, W2 = d_hin.shape
        W = W2 // 2
        assert d_hin.is_contiguous() and mask.is_contiguous() and mask.shape == (bs, O)
        assert d_oin is None or (d_oin.is_contiguous() and d_oin.shape == (bs, T, O, W2))
        d_hfr = torch.empty(bs, T, H, W, dtype=torch.float32, device=d_hin.device)
        d_ofr = torch.empty(bs, T, O, W, dtype=torch.float32, device=d_hin.device)
        d = L.EntityPoolBwd()
        d.d_hin, d.d_oin, d.mask, d.d_hfr, d.d_ofr = d_hin.data_ptr(), _ptr(d_oin), mask.data_ptr(), d_hfr.data_ptr(), d_ofr.data_ptr()
        d.bs, d.T, d.H, d.O, d.W = bs, T, H, O, W
        self._check(self.lib.twog_entity_pool_bwd(C.byref(d), self._stream()), 'twog_entity_pool_bwd')
        return d_hfr, d_ofr

    # ---------------------------------------------------------------- single GRU gate steps (general segment loop)
    @staticmethod
    def _u_fields(g, u):
        """u: None or a (bs, E) view of a (bs, T, E) gate tensor at one time step."""
        if u is None:
            g.u, g.u_ld_outer, g.u_ld_inner, g.u_inner = 0, 0, 0, 1
        else:
            g.u, g.u_ld_outer, g.u_ld_inner, g.u_inner = u.data_ptr(), u.stride(0), u.stride(1), u.shape[1]

    def gru_step_fwd(self, steps):
        """steps: dicts with gi, gi2 (or None), gh, h_prev (or None), h_out, save (row-strided views), u, rows, hidden."""
        arr = (L.GruStep * len(steps))()
        for g, d in zip(arr, steps):
            for k in ('gi', 'gi2', 'gh', 'h_prev', 'h_out', 'save'):
                setattr(g, k, rows_of(d.get(k)))
            self._u_fields(g, d.get('u'))
            g.rows, g.hidden = d['rows'], d['hidden']
        if self._tape is not None:
            self._tape.append((L.TAPE_GRU_STEP_FWD, len(steps), 0, arr))
            return
        self._check(self.lib.twog_gru_step_fwd(arr, len(steps), self._stream()), 'twog_gru_step_fwd')

    GRU_STEP_VEC, GRU_STEP_THREADS_SHIFT, GRU_STEP_LAUNCHES_SHIFT = 1, 4, 16  # TWOG_GRU_STEP_PATH_*

    def gru_step_last_path(self):
        """(16-byte kernel?, workgroup size) of the last chunk the most recent gru_step_fwd call of this thread launched, and
        the number of launches the whole call made (twog_gru_step_last_path)."""
        w = int(self.lib.twog_gru_step_last_path())
        return bool(w & self.GRU_STEP_VEC), (w >> self.GRU_STEP_THREADS_SHIFT) & 0xfff, w >> self.GRU_STEP_LAUNCHES_SHIFT

    def gru_step_bwd(self, steps):
        """steps: dicts with dh, dh2 (or None), save, h_prev (or None), dgi, dgh, dh_prev, u, du (same view form as u)."""
        arr = (L.GruStepBwd * len(steps))()
        for g, d in zip(arr, steps):
            for k in ('dh', 'dh2', 'save', 'h_prev', 'dgi', 'dgh', 'dh_prev'):
                setattr(g, k, rows_of(d.get(k)))
            self._u_fields(g, d.get('u'))
            g.du = _ptr(d.get('du'))
            g.rows, g.hidden, g.dh_prev_accumulate = d['rows'], d['hidden'], int(d.get('dh_prev_accumulate', 0))
        if self._tape is not None:
            self._tape.append((L.TAPE_GRU_STEP_BWD, len(steps), 0, arr))
            return
        self._check(self.lib.twog_gru_step_bwd(arr, len(steps), self._stream()), 'twog_gru_step_bwd')

    # ---------------------------------------------------------------- entity attention
    _ATTN_ROWS = ['feat_h', 'feat_o', 'msg_hh', 'msg_ho', 'msg_oh', 'msg_oo', 'msg_so', 'msg_sh', 'out_hh', 'out_oh',
                  'out_sh', 'out_ho', 'out_so', 'out_oo']

    def _fill_attn(self, a, d):
        for k in self._ATTN_ROWS:
            setattr(a, k, rows_of(d.get(k)))
        a.obj_mask = _ptr(d.get('obj_mask'))
        a.att = _ptr(d.get('att'))
        a.n_inst, a.inst_per_clip, a.H, a.O = d['n_inst'], d['inst_per_clip'], d['H'], d['O']
        a.D, a.hidden, a.scale, a.recv_mask_ho = d['D'], d['hidden'], float(d['scale']), int(d['recv_mask_ho'])

    def attn_fwd(self, descs):
        n = len(descs)
        arr = (L.Attn * n)()
        for i, d in enumerate(descs):
            self._fill_attn(arr[i], d)
        self._check(self.lib.twog_attn_fwd(arr, n, self._stream()), 'twog_attn_fwd')

    def attn_bwd(self, descs):
        n = len(descs)
        arr = (L.AttnBwd * n)()
        for i, d in enumerate(descs):
            self._fill_attn(arr[i].f, d['f'])
            for k in ['dout_hh', 'dout_oh', 'dout_sh', 'dout_ho', 'dout_so', 'dout_oo', 'dmsg_hh', 'dmsg_ho',
                      'dmsg_oh', 'dmsg_oo', 'dmsg_so', 'dmsg_sh', 'dfeat_h', 'dfeat_o']:
                setattr(arr[i], k, rows_of(d.get(k)))
            arr[i].dw_extra = _ptr(d.get('dw_extra'))
            arr[i].dfeat_accumulate = int(d.get('dfeat_accumulate', 0))
            arr[i].relu_mask_dmsg = int(d.get('relu_mask_dmsg', 0))
        self._check(self.lib.twog_attn_bwd(arr, n, self._stream()), 'twog_attn_bwd')

    ATTN_STAGED, ATTN_GRAM_COLUMNS, ATTN_DW_COLUMNS, ATTN_DW_WAVE_GROUPS, ATTN_BACKWARD = 1, 2, 4, 8, 16  # TWOG_ATTN_PATH_*
    ATTN_THREADS_SHIFT = 16

    def attn_last_path(self):
        """Bit field (ATTN_*; workgroup size in the bits from ATTN_THREADS_SHIFT up) of the code path the most recent
        attention launch of this thread selected -- attn_fwd / attn_bwd, or the last step of a launch-per-step segment
        recurrence."""
        return int(self.lib.twog_attn_last_path())

    # ---------------------------------------------------------------- segment-level recurrence
    @staticmethod
    def _seg_dims(p):
        nsh = int(p['rel_hh']) + int(p['rel_ho'])
        nso = int(p['rel_oh']) + int(p['rel_oo'])
        nmh = int(p['rel_hh']) + int(p['rel_oh'])
        nmo = int(p['rel_ho']) + int(p['rel_oo'])
        return nsh, nso, nmh, nmo

    def _fill_seg(self, s, p, bufs):
        s.bs, s.T, s.H, s.O, s.hidden = p['bs'], p['T'], p['H'], p['O'], p['hidden']
        s.msg_segment = int(p['msg_segment'])
        s.rel_hh, s.rel_ho, s.rel_oh, s.rel_oo = (int(p['rel_hh']), int(p['rel_ho']), int(p['rel_oh']),
                                                   int(p['rel_oo']))
        s.att_scale = float(p['att_scale'])
        s.gi_h, s.gi_o, s.u_h, s.u_o = _ptr(p['gi_h']), _ptr(p['gi_o']), _ptr(p['u_h']), _ptr(p['u_o'])
        s.obj_mask = _ptr(p['obj_mask'])
        for d in range(2):
            s.w_hh_h[d], s.b_hh_h[d] = _ptr(p['w_hh_h'][d]), _ptr(p['b_hh_h'][d])
            s.w_hh_o[d], s.b_hh_o[d] = _ptr(p['w_hh_o'][d]), _ptr(p['b_hh_o'][d])
            s.w_ihm_h[d], s.w_ihm_o[d] = _ptr(p['w_ihm_h'][d]), _ptr(p['w_ihm_o'][d])
        s.ld_ih_h, s.ld_ih_o = p['ld_ih_h'], p['ld_ih_o']
        s.w_smsg_h, s.b_smsg_h = _ptr(p.get('w_smsg_h')), _ptr(p.get('b_smsg_h'))
        s.w_smsg_o, s.b_smsg_o = _ptr(p.get('w_smsg_o')), _ptr(p.get('b_smsg_o'))
        for k in ['hs_h', 'hs_o', 'save_h', 'save_o', 'msrc_h', 'msrc_o', 'mg_h', 'mg_o', 'att', 'tmp_gim_h',
                  'tmp_gim_o', 'tmp_gh_h', 'tmp_gh_o', 'zeros']:
            setattr(s, k, _ptr(bufs[k]))

    def segrnn_fwd(self, p):
        """p: parameter/input dict (see ops.SegmentRecurrence). Allocates and returns the state/saved buffers."""
        bs, T, H, O, h = p['bs'], p['T'], p['H'], p['O'], p['hidden']
        dev = p['gi_h'].device if p['gi_h'] is not None else p['gi_o'].device
        nsh, nso, nmh, nmo = self._seg_dims(p)
        natt = H * H + 2 * H * O + O * O

        def e(*shape):
            return torch.empty(*[max(int(x), 0) for x in shape], dtype=torch.float32, device=dev)

        bufs = dict(hs_h=e(bs, T, H, 2 * h), hs_o=e(bs, T, O, 2 * h), save_h=e(2, bs, T, H, 4 * h),
                    save_o=e(2, bs, T, O, 4 * h), msrc_h=e(2, bs, T, H, nsh * h), msrc_o=e(2, bs, T, O, nso * h),
                    mg_h=e(2, bs, T, H, nmh * h), mg_o=e(2, bs, T, O, nmo * h), att=e(2, T, bs, natt),
                    tmp_gim_h=e(2, bs * H, 3 * h), tmp_gim_o=e(2, bs * O, 3 * h), tmp_gh_h=e(2, bs * H, 3 * h),
                    tmp_gh_o=e(2, bs * O, 3 * h),
                    zeros=self.zeros(bs * max(H, O, 1), h, device=dev))
        s = L.SegRnn()
        self._fill_seg(s, p, bufs)
        n_sync = int(self.lib.twog_segrnn_persistent_sync_bytes()) // 4
        self.last_segrnn_persistent = self._try_persistent(   # small batches: the whole recurrence in one launch (csrc/seg_persist.hip)
            'segrnn_fwd', dev, os.environ.get('TWOG_SEG_PERSIST', 'auto'),
            lambda: self.lib.twog_segrnn_persistent_supported(C.byref(s)),
            lambda sync: self.lib.twog_segrnn_fwd_persistent(C.byref(s), sync, self._stream()),
            n_sync=n_sync, err_index=n_sync - 32)
        if not self.last_segrnn_persistent:
            self._check(self.lib.twog_segrnn_fwd(C.byref(s), *self.chain_workspace(dev), self._stream()), 'twog_segrnn_fwd')
        return bufs

    def segrnn_bwd(self, p, bufs, d_hs_h, d_hs_o):
        bs, T, H, O, h = p['bs'], p['T'], p['H'], p['O'], p['hidden']
        dev = bufs['hs_h'].device
        nsh, nso, nmh, nmo = self._seg_dims(p)

        def e(*shape):
            return torch.empty(*[max(int(x), 0) for x in shape], dtype=torch.float32, device=dev)

        d_u_h, d_u_o = self.zeros_many([(bs, T, max(H, 0)), (bs, T, max(O, 0))], dev)
        out = dict(d_gi_h=e(bs, T, H, 6 * h), d_gi_o=e(bs, T, O, 6 * h), d_gh_h=e(bs, T, H, 6 * h),
                   d_gh_o=e(bs, T, O, 6 * h),
                   d_u_h=d_u_h, d_u_o=d_u_o,
                   d_pre_h=e(2, bs, T, H, nsh * h), d_pre_o=e(2, bs, T, O, nso * h))
        scratch = dict(carry_h=e(2, bs * H, h), carry_o=e(2, bs * O, h), tmp_dmg_h=e(2, bs * H, nmh * h),
                       tmp_dmg_o=e(2, bs * O, nmo * h), trash=e(bs * max(H, O, 1), h),
                       du_part_h=e(2, T, 16, bs * H), du_part_o=e(2, T, 16, bs * O))
        s = L.SegRnn()
        self._fill_seg(s, p, bufs)
        b = L.SegRnnBwd()
        b.d_hs_h, b.d_hs_o = _ptr(d_hs_h), _ptr(d_hs_o)
        for k, v in list(out.items()) + list(scratch.items()):
            setattr(b, k, _ptr(v))

        def run(sync):
            scr = self.workspace(int(self.lib.twog_segrnn_bwd_persistent_scratch_bytes(C.byref(s))), dev, 'segp_bwd')
            return self.lib.twog_segrnn_bwd_persistent(C.byref(s), C.byref(b), scr.data_ptr(), scr.numel() * 4, sync, self._stream())

        n_sync = int(self.lib.twog_segrnn_persistent_sync_bytes()) // 4
        self.last_segrnn_bwd_persistent = self._try_persistent(   # small batches: backward through time in one launch
            'segrnn_bwd', dev, os.environ.get('TWOG_SEG_PERSIST', 'auto'),
            lambda: self.lib.twog_segrnn_persistent_supported(C.byref(s)), run, n_sync=n_sync, err_index=n_sync - 32)
        if not self.last_segrnn_bwd_persistent:
            self._check(self.lib.twog_segrnn_bwd(C.byref(s), C.byref(b), *self.chain_workspace(dev), self._stream()), 'twog_segrnn_bwd')
        return out

    def segrnn_persistent_plan(self, bs, T, H, O, h, n_cus=0, msg_segment=True, rels=(True, True, True, True)):
        """What segrnn_fwd / segrnn_bwd would launch persistently for this shape on n_cus compute units (0: the current
        device's): whether it is served, clips per chunk, chunks, the (mh, mo) instance, pair mask, grid, LDS bytes, the
        backward's x3q1 / dw_pad / scratch bytes. Host arithmetic of the library (twog_segrnn_persistent_plan), nothing launched."""
        return L.segrnn_persistent_plan(self.lib, bs, T, H, O, h, n_cus, msg_segment, rels)

    def graph_cache_stats(self):
        """(captured loops, hash-bucket hits resolved by the descriptor compare) of the library's hipGraph cache."""
        n, c = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.twog_graph_cache_stats(C.byref(n), C.byref(c)), 'twog_graph_cache_stats')
        return n.value, c.value

    # ---------------------------------------------------------------- gates
    def _fill_gate(self, g, d):
        g.x = rows_of(d['x'])
        for i, c in enumerate(d['seg_col']):
            g.seg_col[i] = int(c)
        g.n_seg, g.hidden = len(d['seg_col']), d['hidden']
        g.w, g.b, g.noise = _ptr(d['w']), _ptr(d.get('b')), _ptr(d.get('noise'))
        g.hard, g.soft, g.p_save = _ptr(d['hard']), _ptr(d['soft']), _ptr(d['p_save'])
        g.bs, g.T, g.E = d['bs'], d['T'], d['E']
        g.noise_entities, g.noise_offset = int(d.get('noise_entities', 0)), int(d.get('noise_offset', 0))
        g.force_last, g.threshold = int(d['force_last']), float(d['threshold'])

    def gate_fwd(self, d):
        """d: x (rows (bs*T*E), W) view, seg_col, hidden, w, b, noise, bs, T, E, ... Fills d['hard'|'soft'|'p_save']."""
        dev = d['x'].device
        for k in ('hard', 'soft', 'p_save'):
            d[k] = torch.empty(d['bs'], d['T'], d['E'], dtype=torch.float32, device=dev)
        g = L.Gate()
        self._fill_gate(g, d)
        self._check(self.lib.twog_gate_fwd(C.byref(g), self._stream()), 'twog_gate_fwd')
        return d['hard'], d['soft']

    def gate_bwd(self, d, d_hard, d_soft, st_mask):
        g = L.Gate()
        self._fill_gate(g, d)
        dlogit = torch.empty(d['bs'] * d['T'] * d['E'], dtype=torch.float32, device=d['x'].device)
        self._check(self.lib.twog_gate_bwd(C.byref(g), _ptr(d_hard), _ptr(d_soft), _ptr(st_mask), dlogit.data_ptr(),
                                           self._stream()), 'twog_gate_bwd')
        return dlogit

    def new_noise_state(self, seed, calls=0, device=None):
        """The generator state of gumbel_noise_fill: int64 [seed, calls] on `device` (both taken modulo 2^64)."""
        return torch.tensor([_as_int64(seed), _as_int64(calls)], dtype=torch.int64, device=device)

    def gumbel_noise_fill(self, noise, T, noise_entities, bs, clip_offset, state, words=None):
        """noise fp32 (T * noise_entities * bs * 2 values, the layout gate_fwd reads) = the Gumbel noise of call state[1] under
        seed state[0] for the clips clip_offset .. clip_offset + bs - 1 (twog_gumbel_noise_fill: Philox4x32-10, a pure function
        of seed, call, clip, time step and slot); state[1] += 1 on the device behind it. Nothing is read or written on the host.
        words: optional int32 buffer of twice the size that receives the raw generator output. Not a recordable (taped) call:
        issue it before a loop is composed."""
        n = T * noise_entities * bs
        assert noise.dtype == torch.float32 and noise.is_contiguous() and noise.numel() == 2 * n, (tuple(noise.shape), n)
        assert state.dtype == torch.int64 and state.is_contiguous() and state.numel() == 2 and state.device == noise.device
        if words is not None:
            assert words.dtype == torch.int32 and words.is_contiguous() and words.numel() == 4 * n \
                and words.device == noise.device
        if not 0 <= clip_offset < 1 << 32:
            raise ValueError(f'clip_offset {clip_offset} is not a 32-bit unsigned value')
        self._check(self.lib.twog_gumbel_noise_fill(noise.data_ptr(), int(T), int(noise_entities), int(bs), int(clip_offset),
                                                    state.data_ptr(), _ptr(words), self._stream()), 'twog_gumbel_noise_fill')
        return noise

    def augment_grid(self, work):
        """Workgroups of the capped launches of augment_inputs for `work` workgroup-sized items: rows of the feature pass, groups
        of 256 nodes of the geometry pass (twog_augment_grid: host arithmetic of the library, no GPU call)."""
        g = self.lib.twog_augment_grid(int(work))
        if g < 0:
            raise RuntimeError(f'twog_augment_grid failed with code {g}')
        return g

    def augment_inputs(self, x_human, x_objects, clip_ids, state, opts, steps=None, objects_mask=None, params_out=None):
        """In-place augmentation of a batch (twog_augment_inputs, where the arithmetic is stated): x_human (bs, T, H, F_h) whose
        last 4 * opts['gcn_node'] channels are (x, y, vx, vy) nodes, x_objects (bs, T, O, F_o) or None, clip_ids int64 [bs],
        state int64 [seed, epoch] on the device. opts: tan_half_max, scale_max, shift_max, cx, cy, amp, keep_scale,
        drop_threshold, gcn_node (augment.InputAugmentation makes them). Nothing is read or written on the host; neutral options
        launch nothing. Tensors that are not contiguous raise: the write is in place, a silent copy would lose it."""
        dev = x_human.device
        for name, t, dtype in (('x_human', x_human, torch.float32), ('x_objects', x_objects, torch.float32),
                               ('clip_ids', clip_ids, torch.int64), ('state', state, torch.int64), ('steps', steps, torch.float32),
                               ('objects_mask', objects_mask, torch.float32), ('params_out', params_out, torch.float32)):
            if t is None:
                continue
            if t.dtype != dtype or t.device != dev:
                raise TypeError(f'{name}: {t.dtype} on {t.device}, expected {dtype} on {dev}')
            if not t.is_contiguous():
                raise ValueError(f'{name} is not contiguous: augment_inputs writes in place and does not copy')
        if x_human.dim() != 4 or (x_objects is not None and (x_objects.dim() != 4 or x_objects.shape[:2] != x_human.shape[:2])):
            raise ValueError(f'x_human {tuple(x_human.shape)} / x_objects {None if x_objects is None else tuple(x_objects.shape)}')
        bs, T, H, F_h = x_human.shape
        O, F_o = (x_objects.shape[2], x_objects.shape[3]) if x_objects is not None else (0, 0)
        assert clip_ids.numel() == bs and state.numel() == 2
        assert steps is None or steps.numel() == bs
        assert objects_mask is None or objects_mask.numel() == bs * O
        assert params_out is None or params_out.numel() == 4 * bs
        a = L.Augment()
        a.x_human, a.x_objects, a.clip_ids, a.steps = x_human.data_ptr(), _ptr(x_objects), clip_ids.data_ptr(), _ptr(steps)
        a.objects_mask, a.state, a.params_out = _ptr(objects_mask), state.data_ptr(), _ptr(params_out)
        a.bs, a.T, a.H, a.O, a.F_h, a.F_o = bs, T, H, O, F_h, F_o
        a.N, a.geo_offset = int(opts['gcn_node']), F_h - 4 * int(opts['gcn_node'])
        a.tan_half_max, a.scale_max, a.shift_max = opts['tan_half_max'], opts['scale_max'], opts['shift_max']
        a.cx, a.cy, a.amp, a.keep_scale, a.drop_threshold = opts['cx'], opts['cy'], opts['amp'], opts['keep_scale'], \
            int(opts['drop_threshold'])
        self._check(self.lib.twog_augment_inputs(C.byref(a), self._stream()), 'twog_augment_inputs')
        return x_human, x_objects

    def rank1_update(self, dst, s, v):
        """dst[r][c] += s[r] * v[c] on a row-strided view."""
        self._check(self.lib.twog_rank1_update(rows_of(dst), s.data_ptr(), v.data_ptr(), n_rows(dst), dst.shape[-1],
                                               self._stream()), 'twog_rank1_update')

    def colsum(self, x, rowscale=None, out=None, accumulate=False):
        rows, cols = n_rows(x), x.shape[-1]
        if out is None:
            out = torch.empty(cols, dtype=torch.float32, device=x.device)
            accumulate = False
        # enough row slices to fill the chip (~1024 workgroups over column blocks x row slices), >= 64 rows per slice
        nblk = max(1, min(rows // 64, max(1, 1024 // ((cols + 255) // 256))))
        partials = self.workspace(nblk * cols * 4, x.device, 'colsum')
        self._check(self.lib.twog_colsum(rows_of(x), _ptr(rowscale), rows, cols, out.data_ptr(), int(accumulate),
                                         partials.data_ptr(), nblk, self._stream()), 'twog_colsum')
        return out

    def colsum_many(self, ops):
        """ops: (x, rowscale or None, out [cols], accumulate) -- several column sums in one pair of launches (twog_colsum_n);
        each with the arithmetic of its own colsum() call."""
        if not ops:
            return
        arr = (L.ColSum * len(ops))()
        for a, (x, rs, out, acc) in zip(arr, ops):
            assert out.is_contiguous() and out.numel() == x.shape[-1]
            a.x, a.rowscale, a.out = rows_of(x), _ptr(rs), out.data_ptr()
            a.rows, a.cols, a.accumulate = n_rows(x), x.shape[-1], int(bool(acc))
        dev = ops[0][0].device
        need = int(self.lib.twog_colsum_n_partial_floats(arr, len(ops)))
        partials = self.workspace(max(need, 1) * 4, dev, 'colsum')
        self._check(self.lib.twog_colsum_n(arr, len(ops), partials.data_ptr(), partials.numel(), self._stream()), 'twog_colsum_n')

    def filter_fwd(self, soft, threshold):
        bs, T, E = soft.shape
        hard, gmask = torch.empty_like(soft), torch.empty_like(soft)
        self._check(self.lib.twog_filter_fwd(soft.data_ptr(), hard.data_ptr(), gmask.data_ptr(), bs, T, E,
                                             float(threshold), self._stream()), 'twog_filter_fwd')
        return hard, gmask

    # ---------------------------------------------------------------- reorder / heads / elementwise
    def reorder_fwd(self, hx, gate):
        bs, T, E, cols = hx.shape
        assert hx.is_contiguous() and gate.is_contiguous() and gate.shape == (bs, T, E)
        out = torch.empty_like(hx)
        self._check(self.lib.twog_reorder_fwd(hx.data_ptr(), gate.data_ptr(), out.data_ptr(), bs, T, E, cols,
                                              self._stream()), 'twog_reorder_fwd')
        return out

    def reorder_bwd(self, dout, gate):
        bs, T, E, cols = dout.shape
        assert dout.is_contiguous()
        dhx = torch.empty_like(dout)
        self._check(self.lib.twog_reorder_bwd(dout.data_ptr(), gate.data_ptr(), dhx.data_ptr(), bs, T, E, cols,
                                              self._stream()), 'twog_reorder_bwd')
        return dhx

    def logsoftmax_permute_fwd(self, logits, bs, T, E, Cn, out=None):
        """out: a caller-owned (bs, Cn, T, E) buffer. The product never passes one; the parameter exists so that a test can
        hand in a poisoned buffer and see that every position is written and nothing behind the last."""
        if out is None:
            out = torch.empty(bs, Cn, T, E, dtype=torch.float32, device=logits.device)
        assert out.is_contiguous() and out.shape == (bs, Cn, T, E) and out.dtype == torch.float32
        self._check(self.lib.twog_logsoftmax_permute_fwd(logits.data_ptr(), out.data_ptr(), bs, T, E, Cn,
                                                         self._stream()), 'twog_logsoftmax_permute_fwd')
        return out

    def logsoftmax_permute_bwd(self, out, dout):
        bs, Cn, T, E = out.shape
        assert out.is_contiguous() and dout.is_contiguous()
        dlogits = torch.empty(bs * T * E, Cn, dtype=torch.float32, device=out.device)
        self._check(self.lib.twog_logsoftmax_permute_bwd(out.data_ptr(), dout.data_ptr(), dlogits.data_ptr(), bs, T,
                                                         E, Cn, self._stream()), 'twog_logsoftmax_permute_bwd')
        return dlogits

    def relu_bwd(self, dy, y, dx=None):
        """dx = dy * (y > 0) on row-strided views (dx may alias dy)."""
        if dx is None:
            dx = torch.empty(n_rows(dy), dy.shape[-1], dtype=torch.float32, device=dy.device)
        self._check(self.lib.twog_relu_bwd(rows_of(dy), rows_of(y), rows_of(dx), n_rows(dy), dy.shape[-1],
                                           self._stream()), 'twog_relu_bwd')
        return dx

    def add_rows(self, src, dst):
        self._check(self.lib.twog_add_rows(rows_of(src), rows_of(dst), n_rows(src), src.shape[-1], self._stream()),
                    'twog_add_rows')

    # ---------------------------------------------------------------- sender-side projection glue
    def ssp_fwd(self, gi, ph, ps, att, mask, n_inst, inst_per_clip, H, O, att_off):
        """gi (n_inst*O, cols) += mask * (sum_h att[k,h] ph[(inst,h)] + ps[inst]); ph (n_inst*H, cols), ps (n_inst, cols)."""
        cols = gi.shape[-1]
        assert gi.is_contiguous() and (ph is None or ph.is_contiguous()) and (ps is None or ps.is_contiguous())
        natt = att.shape[-1] if att is not None else 0
        self._check(self.lib.twog_ssp_fwd(gi.data_ptr(), _ptr(ph), _ptr(ps), _ptr(att), _ptr(mask), n_inst, inst_per_clip,
                                          H, O, cols, natt, att_off, self._stream()), 'twog_ssp_fwd')

    def ssp_gather(self, dgi, att, att_ld_clip, att_ld_frame, att_off, n_inst, inst_per_clip, H, O):
        """dgi: (n_inst*O, cols) view with unit column stride (row stride free) -> qh (n_inst*H, cols) =
        sum_k att(inst)[att_off + k*H + h] * dgi[(inst, k)]."""
        assert dgi.dim() == 2 and dgi.stride(1) == 1
        cols = dgi.shape[1]
        qh = torch.empty(n_inst * H, cols, dtype=torch.float32, device=dgi.device)
        self._check(self.lib.twog_ssp_gather(dgi.data_ptr(), dgi.stride(0), att.data_ptr(), att_ld_clip, att_ld_frame,
                                             att_off, qh.data_ptr(), n_inst, inst_per_clip, H, O, cols, self._stream()),
                    'twog_ssp_gather')
        return qh

    def ssp_bwd(self, dgi, ph, att, mask, n_inst, inst_per_clip, H, O, att_off, want_qs, dw=None):
        """Returns (qh (n_inst*H, cols) or None, qs (n_inst, cols) or None); fills dw[:, att_off : att_off + O*H] if given."""
        cols = dgi.shape[-1]
        assert dgi.is_contiguous() and (ph is None or ph.is_contiguous())
        qh = torch.empty(n_inst * H, cols, dtype=torch.float32, device=dgi.device) if ph is not None else None
        qs = torch.empty(n_inst, cols, dtype=torch.float32, device=dgi.device) if want_qs else None
        natt = att.shape[-1] if att is not None else 0
        self._check(self.lib.twog_ssp_bwd(dgi.data_ptr(), _ptr(ph), _ptr(att), _ptr(mask), _ptr(qh), _ptr(qs), _ptr(dw),
                                          n_inst, inst_per_clip, H, O, cols, natt, att_off, self._stream()),
                    'twog_ssp_bwd')
        return qh, qs

    # ---------------------------------------------------------------- general single-relation message passing
    REL_SUM, REL_DOT, REL_ADDITIVE, REL_DISTANCE, REL_MEAN = (L.REL_SUM, L.REL_DOT, L.REL_ADDITIVE, L.REL_DISTANCE,
                                                              L.REL_MEAN)
    REL_MSG_SENDER, REL_MSG_PAIR = L.REL_MSG_SENDER, L.REL_MSG_PAIR

    def _fill_relation(self, a, d):
        for k in ('q', 'k', 'msg', 'p_r', 'p_s', 'out'):
            setattr(a, k, rows_of(d.get(k)))
        a.a_r, a.c_s = _ptr(d.get('a_r')), _ptr(d.get('c_s'))
        dist = d.get('dist')   # (n_inst, R, S) view, any strides
        if dist is not None:
            assert dist.dim() == 3 and dist.dtype == torch.float32
            a.dist, (a.dist_ld_inst, a.dist_ld_r, a.dist_ld_s) = dist.data_ptr(), dist.stride()
        else:
            a.dist, a.dist_ld_inst, a.dist_ld_r, a.dist_ld_s = 0, 0, 0, 0
        a.send_mask, a.recv_mask, a.att = _ptr(d.get('send_mask')), _ptr(d.get('recv_mask')), _ptr(d.get('att'))
        a.scale, a.score_bias = float(d.get('scale', 1.0)), _ptr(d.get('score_bias'))
        a.score_mode, a.msg_mode = int(d['score_mode']), int(d['msg_mode'])
        a.relu_scores, a.exclude_self = int(d.get('relu_scores', 0)), int(d.get('exclude_self', 0))
        a.n_inst, a.inst_per_clip, a.R, a.S = d['n_inst'], d['inst_per_clip'], d['R'], d['S']
        a.D, a.hidden = int(d.get('D', 0)), d['hidden']

    def relation_fwd(self, d):
        a = L.Relation()
        self._fill_relation(a, d)
        self._check(self.lib.twog_relation_fwd(C.byref(a), self._stream()), 'twog_relation_fwd')

    def relation_fwd_many(self, ds):
        """Several relations in one call (a few launches of up to 8 descriptors): the general segment loop's level."""
        arr = (L.Relation * len(ds))()
        for a, d in zip(arr, ds):
            self._fill_relation(a, d)
        if self._tape is not None:
            self._tape.append((L.TAPE_RELATION_FWD, len(ds), 0, arr))
            return
        self._check(self.lib.twog_relation_fwd_n(arr, len(ds), self._stream()), 'twog_relation_fwd_n')

    def relation_bwd_many(self, ds):
        """The descriptors must not accumulate (dq / dk) into the same rows: they run concurrently."""
        arr = (L.RelationBwd * len(ds))()
        for b, d in zip(arr, ds):
            self._fill_relation_bwd(b, d)
        if self._tape is not None:
            self._tape.append((L.TAPE_RELATION_BWD, len(ds), 0, arr))
            return
        self._check(self.lib.twog_relation_bwd_n(arr, len(ds), self._stream()), 'twog_relation_bwd_n')

    _ROWOP = {'relu_bwd': 0, 'add': 1, 'rank1': 2}   # TWOG_ROWOP_*

    def rowops(self, ops):
        """ops: ('relu_bwd', dy, y, dx) | ('add', src, dst) | ('rank1', dst, s, v), row-strided views; ONE launch per 16
        operations. No two operations of a call may write the same rows."""
        if not ops:
            return
        arr = (L.RowOp * len(ops))()
        none = rows_of(None)
        for o, op in zip(arr, ops):
            o.kind = self._ROWOP[op[0]]
            if op[0] == 'relu_bwd':
                _, dy, y, dst = op
                o.a, o.b = rows_of(dy), rows_of(y)
            elif op[0] == 'add':
                _, src, dst = op
                o.a, o.b = rows_of(src), none
            else:
                _, dst, sv, v = op
                assert sv.is_contiguous() and v.is_contiguous() and sv.numel() == n_rows(dst) and v.numel() == dst.shape[-1]
                o.a, o.b, o.s, o.v = none, none, sv.data_ptr(), v.data_ptr()
            o.dst, o.rows, o.cols = rows_of(dst), n_rows(dst), dst.shape[-1]
        if self._tape is not None:
            self._tape.append((L.TAPE_ROWOPS, len(ops), 0, arr))
            return
        self._check(self.lib.twog_rowops(arr, len(ops), self._stream()), 'twog_rowops')

    # ---------------------------------------------------------------- recorded steps of an affine loop (twog_tape_run)
    def tape_begin(self):
        """From here to tape_end(), gemm / gru_step_* / relation_*_many / rowops calls are RECORDED (descriptor arrays
        kept, nothing issued). Any other entry point called in between is a programming error the recording cannot see:
        the general segment loop (ops.segment_recurrence_general_*) uses only these six."""
        assert self._tape is None
        self._tape = []

    def tape_end(self):
        t, self._tape = self._tape, None
        return t

    @staticmethod
    def tape_predict(a, b, k):
        """The descriptor bytes twog_tape_run builds for step a + k: per 64-bit word a + k (b - a). For checking a third
        composed step against the rule before trusting it with the rest of the loop."""
        import numpy as np
        out = []
        for (ka, na, fa, da), (kb, nb, fb, db) in zip(a, b):
            wa = np.frombuffer(bytes(da), dtype=np.uint64)
            wb = np.frombuffer(bytes(db), dtype=np.uint64)
            out.append((wa + np.uint64(k) * (wb - wa)).tobytes())
        return out

    @staticmethod
    def tape_same_program(a, b):
        return len(a) == len(b) and all(x[:3] == y[:3] for x, y in zip(a, b))

    def tape_matches(self, a, b, c, k):
        """True if the composed step c is what the replay would run as step a + k."""
        if not (self.tape_same_program(a, b) and self.tape_same_program(a, c)):
            return False
        return all(bytes(e[3]) == w for e, w in zip(c, self.tape_predict(a, b, k)))

    def tape_run(self, a, b, k_begin, k_end, device):
        """Issues steps a + k, k_begin <= k < k_end, of the loop whose consecutive steps a and b were recorded."""
        assert self._tape is None and self.tape_same_program(a, b)
        n = len(a)
        ea, eb = (L.TapeEntry * n)(), (L.TapeEntry * n)()
        for arr, tape in ((ea, a), (eb, b)):
            for e, (kind, cnt, flags, desc) in zip(arr, tape):
                e.kind, e.n, e.flags, e.desc = kind, cnt, flags, C.addressof(desc)
        ws = self.workspace(320 << 20, device, 'splitk')
        self._check(self.lib.twog_tape_run(ea, eb, n, k_begin, k_end, ws.data_ptr(), ws.numel() * 4, self._stream()),
                    'twog_tape_run')

    def relation_bwd(self, d):
        """d: dict(f=<forward descriptor>, dout, dmsg | dp_r, dp_s, dq, dk, da_r, dc_s, dq_accumulate, ...)."""
        b = L.RelationBwd()
        self._fill_relation_bwd(b, d)
        self._check(self.lib.twog_relation_bwd(C.byref(b), self._stream()), 'twog_relation_bwd')

    def _fill_relation_bwd(self, b, d):
        self._fill_relation(b.f, d['f'])
        for k in ('dout', 'dmsg', 'dp_r', 'dp_s', 'dq', 'dk'):
            setattr(b, k, rows_of(d.get(k)))
        b.da_r, b.dc_s, b.dscore_sum = _ptr(d.get('da_r')), _ptr(d.get('dc_s')), _ptr(d.get('dscore_sum'))
        b.dq_accumulate, b.dk_accumulate = int(d.get('dq_accumulate', 0)), int(d.get('dk_accumulate', 0))
        b.relu_mask_dmsg = int(d.get('relu_mask_dmsg', 0))

    # ---------------------------------------------------------------- position features / rare gate strategies
    def pos_embed_fwd(self, out, bs, T, E, hidden, w=None, b=None, periodic=False, s=None, steps=None, divide=False):
        """out: (bs*T*E, hidden) row-strided view (a column block of the entity rows). Returns the scalars [bs*T*E]."""
        s_out = torch.empty(bs * T * E, dtype=torch.float32, device=out.device)
        self._check(self.lib.twog_pos_embed_fwd(_ptr(s), _ptr(steps), bs, T, E, int(divide), _ptr(w), _ptr(b),
                                                int(periodic), hidden, rows_of(out), s_out.data_ptr(), self._stream()),
                    'twog_pos_embed_fwd')
        return s_out

    def periodic_embed_bwd(self, dout, s):
        ds = torch.empty(n_rows(dout), dtype=torch.float32, device=dout.device)
        self._check(self.lib.twog_periodic_embed_bwd(rows_of(dout), s.data_ptr(), n_rows(dout), dout.shape[-1],
                                                     ds.data_ptr(), self._stream()), 'twog_periodic_embed_bwd')
        return ds

    def seglen_fwd(self, u, steps, divide):
        bs, T, E = u.shape
        assert u.is_contiguous()
        s = torch.empty(bs, T, E, dtype=torch.float32, device=u.device)
        self._check(self.lib.twog_seglen_fwd(u.data_ptr(), _ptr(steps), bs, T, E, int(divide), s.data_ptr(),
                                             self._stream()), 'twog_seglen_fwd')
        return s

    def seglen_bwd(self, u, steps, divide, ds, du):
        """du (bs, T, E) += d(segment lengths)/d(hard gates) applied to ds."""
        bs, T, E = u.shape
        assert ds.is_contiguous() and du.is_contiguous()
        self._check(self.lib.twog_seglen_bwd(u.data_ptr(), _ptr(steps), bs, T, E, int(divide), ds.data_ptr(),
                                             du.data_ptr(), self._stream()), 'twog_seglen_bwd')

    def mul(self, a, b, out=None, accumulate=False):
        assert a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel()
        if out is None:
            out, accumulate = torch.empty_like(a), False
        assert out.is_contiguous()
        self._check(self.lib.twog_mul(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), int(accumulate),
                                      self._stream()), 'twog_mul')
        return out

    def scale_rows(self, x, s):
        self._check(self.lib.twog_scale_rows(rows_of(x), s.data_ptr(), n_rows(x), x.shape[-1], self._stream()),
                    'twog_scale_rows')

    def adam_step(self, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
        self._check(self.lib.twog_adam_step(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(),
                                            exp_avg_sq.data_ptr(), param.numel(), lr, beta1, beta2, eps, weight_decay,
                                            step, grad_scale, self._stream()), 'twog_adam_step')

    # ---------------------------------------------------------------- training-step options (csrc/train_opts.hip)
    def grad_norm(self, buf, ranges, scale, max_norm, out=None):
        """Global L2 norm of buf[b:e] for (b, e) in ranges, times |scale|, and the clip coefficient
        max_norm / (norm + 1e-6): out [2] fp32 = (norm, coef), on the device (no host read)."""
        assert buf.dtype == torch.float32 and buf.dim() == 1 and buf.is_contiguous()
        ranges = [(int(b), int(e)) for b, e in ranges]
        if len(ranges) > L.NORM_MAX_RANGES:
            raise ValueError(f'at most {L.NORM_MAX_RANGES} ranges per call')
        R = L.Ranges()
        for i, (b, e) in enumerate(ranges):
            if not 0 <= b <= e <= buf.numel():
                raise ValueError(f'range {(b, e)} outside a buffer of {buf.numel()} elements')
            R.begin[i], R.end[i] = b, e
        R.n_ranges = len(ranges)
        if out is None:
            out = torch.empty(2, dtype=torch.float32, device=buf.device)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= 2
        partials = self.workspace(L.NORM_BLOCKS * 8, buf.device, 'norm')
        self._check(self.lib.twog_grad_norm(buf.data_ptr(), C.byref(R), float(scale), float(max_norm), partials.data_ptr(),
                                            out.data_ptr(), self._stream()), 'twog_grad_norm')
        return out

    def adam_step_coef(self, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                       coef):
        """adam_step with the gradient multiplied by min(coef[0], 1) (coef: a device fp32 scalar; NaN: no clipping)."""
        n = param.numel()
        assert grad.numel() == exp_avg.numel() == exp_avg_sq.numel() == n and coef.dtype == torch.float32
        self._check(self.lib.twog_adam_step_coef(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(),
                                                 exp_avg_sq.data_ptr(), n, lr, beta1, beta2, eps, weight_decay, step,
                                                 grad_scale, coef.data_ptr(), self._stream()), 'twog_adam_step_coef')

    # ---------------------------------------------------------------- Adam with its step state on the device
    STREAM_OPTIM = 13   # TWOG_STREAM_OPTIM (twog_stream_grid; 12 is not assigned)
    OPTIM_CLIP, OPTIM_DECOUPLED, OPTIM_SKIP_NONFINITE = L.OPTIM_CLIP, L.OPTIM_DECOUPLED, L.OPTIM_SKIP_NONFINITE

    def new_optim_state(self, step, skipped, beta1, beta2, device, powers=None):
        """The 64-byte twog_optim_state_t as a uint8 [64] tensor on `device` (optim_state_block: the powers by `step` fp64
        multiplications on the host unless given)."""
        return optim_state_block(step, skipped, beta1, beta2, powers).to(device)

    def optim_prepare(self, state, hyper, lr, norms=(), coef=None, flags=0):
        """twog_optim_prepare: advances the state block by one step, or counts a skipped one. hyper: dict(beta1, beta2, eps,
        weight_decay, grad_scale, ema_decay); lr: a float or a one-element fp32 device tensor (read by the launch); norms: up to two
        one-element fp32 device tensors (twog_grad_norm's out[0:1]); coef: the clip coefficient (out[1:2]) or None."""
        _check_optim_state(state)
        lr_t = lr if torch.is_tensor(lr) else None
        for t in list(norms) + [coef, lr_t]:
            assert t is None or (t.dtype == torch.float32 and t.numel() >= 1 and t.device == state.device)
        arr = (C.c_void_p * 2)(*[t.data_ptr() for t in norms]) if len(norms) <= 2 else None
        self._check(self.lib.twog_optim_prepare(state.data_ptr(), C.byref(optim_hyper(hyper)), 0.0 if lr_t is not None else float(lr),
                                                _ptr(lr_t), arr, len(norms), _ptr(coef), int(flags), self._stream()),
                    'twog_optim_prepare')

    def optim_apply(self, param, grad, exp_avg, exp_avg_sq, ema, hyper, flags, state):
        """twog_optim_apply over param.numel() elements (contiguous fp32 views at the same offset of equally aligned buffers);
        ema: the averaged weights or None. Writes nothing when the prepared step is a skipped one."""
        _check_optim_state(state)
        n = param.numel()
        for t in (param, grad, exp_avg, exp_avg_sq, ema):
            assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n and t.device == state.device)
        self._check(self.lib.twog_optim_apply(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                              _ptr(ema), n, C.byref(optim_hyper(hyper)), int(flags), state.data_ptr(),
                                              self._stream()), 'twog_optim_apply')

    @staticmethod
    def _mtl_spec(kinds):
        if len(kinds) > L.MTL_MAX_TERMS:
            raise ValueError(f'at most {L.MTL_MAX_TERMS} loss terms')
        spec = L.Mtl()
        for i, k in enumerate(kinds):
            spec.kind[i] = int(k)
        spec.n = len(kinds)
        return spec

    def mtl_weight_fwd(self, kinds, losses, log_sds):
        """The multi-task loss learner's forward over [n] losses (kinds: MTL_PASS / _SOFTMAX / _MSE / _MAE per term)."""
        assert losses.is_contiguous() and log_sds.is_contiguous() and losses.numel() == log_sds.numel() == len(kinds)
        out = torch.empty_like(losses)
        self._check(self.lib.twog_mtl_weight_fwd(C.byref(self._mtl_spec(kinds)), losses.data_ptr(), log_sds.data_ptr(),
                                                 out.data_ptr(), self._stream()), 'twog_mtl_weight_fwd')
        return out

    def mtl_weight_bwd(self, kinds, losses, log_sds, dout, dlog_sds, accumulate):
        """Returns d(losses) [n]; d(log_sds) is added into (accumulate) or stored in `dlog_sds`."""
        dout = dout.contiguous()
        assert dlog_sds.is_contiguous() and dlog_sds.numel() == len(kinds)
        dlosses = torch.empty_like(losses)
        self._check(self.lib.twog_mtl_weight_bwd(C.byref(self._mtl_spec(kinds)), losses.data_ptr(), log_sds.data_ptr(),
                                                 dout.data_ptr(), dlosses.data_ptr(), dlog_sds.data_ptr(), int(accumulate),
                                                 self._stream()), 'twog_mtl_weight_bwd')
        return dlosses


    # ---------------------------------------------------------------- multi-task loss
    def _loss_terms(self, terms, dinputs=None, struct=L.Loss):
        """terms: list of dict(kind 0 NLL / 1 BCE / 2 budget, input, target, weight, ignore). input/target contiguous.
        struct=L.WLoss reads two more keys: class_weight (contiguous fp32 [n_classes] on the input's device, or None; NLL
        terms only) and positive_class_weight (a number; BCE terms only)."""
        arr = (struct * len(terms))()
        for i, (t, a) in enumerate(zip(terms, arr)):
            if struct is L.WLoss:
                cw, p = t.get('class_weight'), float(t.get('positive_class_weight', 1.0))
                assert cw is None or t['kind'] == 0, 'class_weight on a term that is not NLL'
                assert p == 1.0 or t['kind'] == 1, 'positive_class_weight on a term that is not BCE'
                if cw is not None:
                    x = t['input']
                    assert cw.dtype == torch.float32 and cw.is_contiguous() and cw.device == x.device
                    assert cw.dim() == 1 and cw.numel() == x.shape[1], (tuple(cw.shape), tuple(x.shape))
                a.class_weight, a.positive_class_weight = _ptr(cw), p
            x, y = t['input'], t['target']
            assert x.is_contiguous() and y.is_contiguous() and x.dtype == torch.float32
            a.kind = t['kind']
            if t['kind'] == 0:
                assert y.dtype == torch.int64 and x.dim() >= 2 and y.numel() * x.shape[1] == x.numel()
                a.n_classes, a.outer = x.shape[1], x.shape[0]
                a.inner = x.numel() // max(x.shape[0] * x.shape[1], 1)
            else:
                assert y.dtype == torch.float32 and y.numel() == x.numel()
                a.n_classes, a.outer, a.inner = 1, 1, x.numel()
            a.input, a.target = x.data_ptr(), y.data_ptr()
            a.dinput = None if dinputs is None or dinputs[i] is None else dinputs[i].data_ptr()
            a.weight, a.ignore_value = float(t['weight']), float(t['ignore'])
        return arr

    def _criterion_fwd(self, entry, struct, terms, room):
        n, dev = len(terms), terms[0]['input'].device
        if n > L.LOSS_MAX_TERMS:
            raise ValueError(f'at most {L.LOSS_MAX_TERMS} loss terms per call')
        losses = torch.empty(n + room, dtype=torch.float32, device=dev)
        stats = torch.empty(n + room, 2, dtype=torch.float64, device=dev)
        partials = self.workspace(n * L.LOSS_BLOCKS * 2 * 8, dev, 'loss')
        self._check(getattr(self.lib, entry)(self._loss_terms(terms, struct=struct), n, partials.data_ptr(), stats.data_ptr(),
                                             losses.data_ptr(), self._stream()), entry)
        return losses, stats

    def _criterion_bwd(self, entry, struct, terms, stats, dlosses, need):
        dins = [torch.empty_like(t['input']) if nd else None for t, nd in zip(terms, need)]
        self._check(getattr(self.lib, entry)(self._loss_terms(terms, dins, struct=struct), len(terms), stats.data_ptr(),
                                             dlosses.contiguous().data_ptr(), self._stream()), entry)
        return dins

    def multitask_loss_fwd(self, terms, room=0):
        """All loss terms in one launch. Returns (losses [n + room] fp32, stats [n + room][2] fp64 = sum, count): the first n
        rows are written here, the `room` rows behind them are left to smooth_loss_fwd, so the criterion's losses stay ONE
        tensor (multi_task._loss_tensor reads it in place) without a copy."""
        return self._criterion_fwd('twog_multitask_loss_fwd', L.Loss, terms, room)

    def multitask_loss_bwd(self, terms, stats, dlosses, need):
        """d(input) of every term with need[i] (others None), scaled by the upstream gradient dlosses [n]."""
        return self._criterion_bwd('twog_multitask_loss_bwd', L.Loss, terms, stats, dlosses, need)

    def weighted_loss_fwd(self, terms, room=0):
        """multitask_loss_fwd for terms that may carry `class_weight` (NLL) and `positive_class_weight` (BCE), through
        twog_weighted_loss_fwd: same returns, stats = (sum, den) with den the sum of the kept class weights of an NLL term."""
        return self._criterion_fwd('twog_weighted_loss_fwd', L.WLoss, terms, room)

    def weighted_loss_bwd(self, terms, stats, dlosses, need):
        """multitask_loss_bwd for the terms of weighted_loss_fwd."""
        return self._criterion_bwd('twog_weighted_loss_bwd', L.WLoss, terms, stats, dlosses, need)

    @staticmethod
    def _check_tail(m, losses, stats, dins=None, shared=None):
        """The views of a tail family of m terms: losses (or dlosses) [m] fp32 and stats [m][2] fp64, contiguous; and no two
        of its gradient buffers `dins` the same (`shared`: the assertion text)."""
        assert losses.shape == (m,) and losses.dtype == torch.float32 and losses.is_contiguous()
        assert stats.shape == (m, 2) and stats.dtype == torch.float64 and stats.is_contiguous()
        if dins is not None:
            ptrs = [d.data_ptr() for d in dins if d is not None]
            assert len(set(ptrs)) == len(ptrs), shared

    def _smooth_terms(self, terms, dinputs=None, accumulate=None):
        """terms: list of dict(input (outer, C, T, E) log-probabilities, target int64 (outer, T, E), weight, tau, ignore)."""
        if len(terms) > L.LOSS_MAX_TERMS:
            raise ValueError(f'at most {L.LOSS_MAX_TERMS} smoothing terms per call')
        arr = (L.SmoothLoss * len(terms))()
        for i, (t, a) in enumerate(zip(terms, arr)):
            x, y = t['input'], t['target']
            assert x.is_contiguous() and y.is_contiguous() and x.dtype == torch.float32 and y.dtype == torch.int64
            assert x.dim() == 4 and y.shape == (x.shape[0], x.shape[2], x.shape[3]), (tuple(x.shape), tuple(y.shape))
            a.outer, a.n_classes, a.steps, a.entities = x.shape
            a.input, a.target = x.data_ptr(), y.data_ptr()
            a.dinput = None
            if dinputs is not None and dinputs[i] is not None:
                d = dinputs[i]
                assert d.is_contiguous() and d.dtype == torch.float32 and d.shape == x.shape and d.device == x.device
                a.dinput, a.accumulate = d.data_ptr(), int(bool(accumulate[i]))
            a.weight, a.tau, a.ignore_value = float(t['weight']), float(t['tau']), float(t['ignore'])
        return arr

    def smooth_loss_fwd(self, terms, losses_out, stats_out):
        """The temporal smoothing terms (twog_smooth_loss_t) in one launch pair, written into the given views: losses_out
        [m] fp32 and stats_out [m][2] fp64, the tail of the tensors multitask_loss_fwd(..., room=m) returned."""
        m, dev = len(terms), terms[0]['input'].device
        self._check_tail(m, losses_out, stats_out)
        assert losses_out.device == dev and stats_out.device == dev
        partials = self.workspace(m * L.LOSS_BLOCKS * 2 * 8, dev, 'smooth_loss')
        self._check(self.lib.twog_smooth_loss_fwd(self._smooth_terms(terms), m, partials.data_ptr(), stats_out.data_ptr(),
                                                  losses_out.data_ptr(), self._stream()), 'twog_smooth_loss_fwd')

    def smooth_loss_bwd(self, terms, stats, dlosses, dins, accumulate):
        """d(input) of every smoothing term with a buffer in dins (None: skipped), scaled by dlosses [m]: stored into dins[i]
        (every element), or with accumulate[i] added where it is not zero. No two terms may share a buffer."""
        m = len(terms)
        self._check_tail(m, dlosses, stats, dins, 'two smoothing terms of one launch share a gradient buffer')
        self._check(self.lib.twog_smooth_loss_bwd(self._smooth_terms(terms, dins, accumulate), m, stats.data_ptr(),
                                                  dlosses.data_ptr(), self._stream()), 'twog_smooth_loss_bwd')

    # ---------------------------------------------------------------- linear-chain CRF loss
    def crf_limits(self):
        """(largest class count, most model steps) the CRF loss takes: those of viterbi_limits."""
        max_classes, max_steps = C.c_int(0), C.c_int(0)
        self._check(self.lib.twog_crf_limits(C.byref(max_classes), C.byref(max_steps)), 'twog_crf_limits')
        return max_classes.value, max_steps.value

    def crf_workspace(self, bs, num_classes, T, E):
        """Bytes of the (alpha, seq, partials) workspaces of a CRF term of this shape. Launch-free; ValueError beyond
        crf_limits."""
        return L.crf_workspace(self.lib, bs, num_classes, T, E)

    def _crf_term(self, t):
        """A CRF term: dict(input (bs, C, T, E) fp32 log-probabilities, target int64 (bs, T, E), transitions fp32 (C, C),
        initial fp32 (C,), weight, ignore). Returns its shape; ValueError beyond crf_limits."""
        x, y, A, pi = t['input'], t['target'], t['transitions'], t['initial']
        assert x.is_contiguous() and y.is_contiguous() and x.dtype == torch.float32 and y.dtype == torch.int64
        assert x.dim() == 4 and y.shape == (x.shape[0], x.shape[2], x.shape[3]), (tuple(x.shape), tuple(y.shape))
        bs, Cn, T, E = x.shape
        max_classes, max_steps = self.crf_limits()
        if Cn > max_classes or T > max_steps:
            raise ValueError(f'the CRF loss takes up to {max_classes} classes and {max_steps} model steps, not {Cn} and {T}')
        for p, shape in ((A, (Cn, Cn)), (pi, (Cn,))):
            assert p.shape == shape and p.dtype == torch.float32 and p.is_contiguous() and p.device == x.device, \
                (tuple(p.shape), p.dtype, p.device)
        return bs, Cn, T, E

    def crf_nll_fwd(self, terms, losses_out, stats_out):
        """The CRF terms (twog_crf_nll_fwd in include/twog_gcn.h), one launch pair each, written into the given views:
        losses_out [m] fp32 and stats_out [m][2] fp64 = (sum of nll_seq, kept steps), the tail of the tensors
        multitask_loss_fwd(..., room=) returned. Every term keeps its 'alpha' and 'seq' workspaces for crf_nll_bwd;
        seq (bs * E, 4) fp32 holds logZ, gold, nll_seq and K (the bits of an int32) per sequence."""
        m = len(terms)
        shapes = [self._crf_term(t) for t in terms]   # every refusal before the first launch
        self._check_tail(m, losses_out, stats_out)
        for j, (t, (bs, Cn, T, E)) in enumerate(zip(terms, shapes)):
            x = t['input']
            assert losses_out.device == x.device and stats_out.device == x.device
            if T == 0 or E == 0:
                bs = 0   # no sequence: the sums alone, over nothing
            alpha_bytes, seq_bytes, _ = self.crf_workspace(bs, Cn, max(T, 1), max(E, 1))
            t['alpha'] = torch.empty(alpha_bytes // 4, dtype=torch.float32, device=x.device)
            t['seq'] = torch.empty(seq_bytes // 4 // L.CRF_SEQ_WORDS, L.CRF_SEQ_WORDS, dtype=torch.float32, device=x.device)
            self._check(self.lib.twog_crf_nll_fwd(x.data_ptr(), t['target'].data_ptr(), bs, Cn, max(T, 1), max(E, 1),
                                                  t['transitions'].data_ptr(), t['initial'].data_ptr(), int(t['ignore']),
                                                  float(t['weight']), t['alpha'].data_ptr(), t['seq'].data_ptr(),
                                                  stats_out[j].data_ptr(), losses_out[j:].data_ptr(), self._stream()),
                        'twog_crf_nll_fwd')

    def crf_nll_bwd(self, terms, stats, dlosses, dins, accumulate, need_params):
        """The gradients of the CRF terms of crf_nll_fwd, scaled by dlosses [m]. d(input) of term j is stored into dins[j]
        (every element), or with accumulate[j] added to it; dins[j] None: not asked for. need_params[j]: also (dA, dpi) of
        the term, new tensors. Returns the list of (dA, dpi) or None per term. A term that asks for neither is skipped."""
        m = len(terms)
        self._check_tail(m, dlosses, stats, dins, 'two CRF terms share a gradient buffer')
        out = []
        for j, t in enumerate(terms):
            d, want = dins[j], bool(need_params[j])
            if d is None and not want:
                out.append(None)
                continue
            x = t['input']
            bs, Cn, T, E = x.shape
            if d is not None:
                assert d.is_contiguous() and d.dtype == torch.float32 and d.shape == x.shape and d.device == x.device
            if T == 0 or E == 0:
                bs = 0
            dA = dpi = partials = None
            if want:
                dA = torch.empty(Cn, Cn, dtype=torch.float32, device=x.device)
                dpi = torch.empty(Cn, dtype=torch.float32, device=x.device)
                partials = self.workspace(self.crf_workspace(bs, Cn, max(T, 1), max(E, 1))[2], x.device, 'crf_partials')
            self._check(self.lib.twog_crf_nll_bwd(x.data_ptr(), t['target'].data_ptr(), bs, Cn, max(T, 1), max(E, 1),
                                                  t['transitions'].data_ptr(), int(t['ignore']), float(t['weight']),
                                                  t['alpha'].data_ptr(), t['seq'].data_ptr(), stats[j].data_ptr(),
                                                  dlosses[j:].data_ptr(), _ptr(d), int(bool(accumulate[j])), _ptr(partials),
                                                  _ptr(dA), _ptr(dpi), 0, self._stream()), 'twog_crf_nll_bwd')
            out.append((dA, dpi) if want else None)
        return out

    # ---------------------------------------------------------------- semi-Markov CRF loss
    def semicrf_limits(self):
        """(largest class count, most model steps, longest duration) the semi-Markov CRF loss takes: those of
        segdecode_limits."""
        max_classes, max_steps, max_duration = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.lib.twog_semicrf_limits(C.byref(max_classes), C.byref(max_steps), C.byref(max_duration)),
                    'twog_semicrf_limits')
        return max_classes.value, max_steps.value, max_duration.value

    def semicrf_plan(self, bs, num_classes, T, E, D):
        """The launches and workspaces of a semi-Markov CRF term of this shape (twog_semicrf_plan) as a dict: class_template,
        fwd_waves, fwd_groups, bwd_waves, bwd_groups, ed_bytes, marks_bytes, seq_bytes, partial_bytes. Launch-free;
        ValueError beyond semicrf_limits."""
        return L.semicrf_plan(self.lib, bs, num_classes, T, E, D)

    def _semicrf_term(self, t):
        """A semi-Markov CRF term: a CRF term's dict with durations fp32 (C, D) beside transitions and initial. Returns its
        shape and D; ValueError beyond semicrf_limits."""
        x, y, A, pi, dur = t['input'], t['target'], t['transitions'], t['initial'], t['durations']
        assert x.is_contiguous() and y.is_contiguous() and x.dtype == torch.float32 and y.dtype == torch.int64
        assert x.dim() == 4 and y.shape == (x.shape[0], x.shape[2], x.shape[3]), (tuple(x.shape), tuple(y.shape))
        bs, Cn, T, E = x.shape
        assert dur.dim() == 2 and dur.shape[1] >= 1, tuple(dur.shape)
        D = dur.shape[1]
        max_classes, max_steps, max_duration = self.semicrf_limits()
        if Cn > max_classes or T > max_steps or D > max_duration:
            raise ValueError(f'the semi-Markov CRF loss takes up to {max_classes} classes, {max_steps} model steps and '
                             f'durations up to {max_duration}, not {Cn}, {T} and {D}')
        for p, shape in ((A, (Cn, Cn)), (pi, (Cn,)), (dur, (Cn, D))):
            assert p.shape == shape and p.dtype == torch.float32 and p.is_contiguous() and p.device == x.device, \
                (tuple(p.shape), p.dtype, p.device)
        return bs, Cn, T, E, D

    def semicrf_nll_fwd(self, terms, losses_out, stats_out):
        """The semi-Markov CRF terms (twog_semicrf_nll_fwd in include/twog_gcn.h), one launch pair each, written into the
        given views as crf_nll_fwd writes them. Every term keeps its 'ed', 'marks' and 'seq' workspaces for semicrf_nll_bwd;
        seq (bs * E, 4) fp32 holds logZ, gold, nll_seq and K (the bits of an int32) per sequence."""
        m = len(terms)
        shapes = [self._semicrf_term(t) for t in terms]   # every refusal before the first launch
        self._check_tail(m, losses_out, stats_out)
        for j, (t, (bs, Cn, T, E, D)) in enumerate(zip(terms, shapes)):
            x = t['input']
            assert losses_out.device == x.device and stats_out.device == x.device
            if T == 0 or E == 0:
                bs = 0   # no sequence: the sums alone, over nothing
            plan = self.semicrf_plan(bs, Cn, max(T, 1), max(E, 1), D)
            t['ed'] = torch.empty(plan['ed_bytes'] // 4, dtype=torch.float32, device=x.device)
            t['marks'] = torch.empty(plan['marks_bytes'] // 4, dtype=torch.int32, device=x.device)
            t['seq'] = torch.empty(plan['seq_bytes'] // 4 // L.SEMICRF_SEQ_WORDS, L.SEMICRF_SEQ_WORDS, dtype=torch.float32,
                                   device=x.device)
            self._check(self.lib.twog_semicrf_nll_fwd(x.data_ptr(), t['target'].data_ptr(), bs, Cn, max(T, 1), max(E, 1),
                                                      t['transitions'].data_ptr(), t['initial'].data_ptr(),
                                                      t['durations'].data_ptr(), D, int(t['ignore']), float(t['weight']),
                                                      t['ed'].data_ptr(), t['marks'].data_ptr(), t['seq'].data_ptr(),
                                                      stats_out[j].data_ptr(), losses_out[j:].data_ptr(), self._stream()),
                        'twog_semicrf_nll_fwd')

    def semicrf_nll_bwd(self, terms, stats, dlosses, dins, accumulate, need_params):
        """The gradients of the terms of semicrf_nll_fwd, scaled by dlosses [m]: as crf_nll_bwd, with (dA, dpi, ddur) per
        term whose parameters are asked for."""
        m = len(terms)
        self._check_tail(m, dlosses, stats, dins, 'two semi-Markov CRF terms share a gradient buffer')
        out = []
        for j, t in enumerate(terms):
            d, want = dins[j], bool(need_params[j])
            if d is None and not want:
                out.append(None)
                continue
            x = t['input']
            bs, Cn, T, E = x.shape
            D = t['durations'].shape[1]
            if d is not None:
                assert d.is_contiguous() and d.dtype == torch.float32 and d.shape == x.shape and d.device == x.device
            if T == 0 or E == 0:
                bs = 0
            dA = dpi = ddur = partials = None
            if want:
                dA = torch.empty(Cn, Cn, dtype=torch.float32, device=x.device)
                dpi = torch.empty(Cn, dtype=torch.float32, device=x.device)
                ddur = torch.empty(Cn, D, dtype=torch.float32, device=x.device)
                partials = self.workspace(self.semicrf_plan(bs, Cn, max(T, 1), max(E, 1), D)['partial_bytes'], x.device,
                                          'semicrf_partials')
            self._check(self.lib.twog_semicrf_nll_bwd(x.data_ptr(), t['target'].data_ptr(), bs, Cn, max(T, 1), max(E, 1),
                                                      t['transitions'].data_ptr(), t['durations'].data_ptr(), D,
                                                      int(t['ignore']), float(t['weight']), t['ed'].data_ptr(),
                                                      t['marks'].data_ptr(), t['seq'].data_ptr(), stats[j].data_ptr(),
                                                      dlosses[j:].data_ptr(), _ptr(d), int(bool(accumulate[j])), _ptr(partials),
                                                      _ptr(dA), _ptr(dpi), _ptr(ddur), 0, self._stream()),
                        'twog_semicrf_nll_bwd')
            out.append((dA, dpi, ddur) if want else None)
        return out


    # ---------------------------------------------------------------- inference post-processing
    def predict_labels(self, logp, downsampling, target_steps):
        """(bs, C, T, E) log-probabilities -> int64 labels (bs, target_steps, E) (upsample, match_shape, argmax)."""
        assert logp.dim() == 4 and logp.dtype == torch.float32
        logp = logp.contiguous()
        bs, Cn, T, E = logp.shape
        labels = torch.empty(bs, target_steps, E, dtype=torch.int64, device=logp.device)
        self._check(self.lib.twog_predict_labels(logp.data_ptr(), bs, Cn, T, E, int(downsampling), int(target_steps),
                                                 labels.data_ptr(), self._stream()), 'twog_predict_labels')
        return labels

    def f1_at_k(self, y_true, y_pred, num_classes, overlap, ignore_value=None):
        """Per-sequence F1@k and validity flags for int64 (n_seq, n_steps) label matrices."""
        y_true, y_pred = y_true.to(torch.int64).contiguous(), y_pred.to(torch.int64).contiguous()
        n_seq, n_steps = y_true.shape
        dev = y_true.device
        f1 = torch.zeros(n_seq, dtype=torch.float32, device=dev)
        valid = torch.zeros(n_seq, dtype=torch.float32, device=dev)
        scratch = torch.empty(max(n_seq * n_steps, 1), dtype=torch.uint8, device=dev)
        self._check(self.lib.twog_f1_at_k(y_true.data_ptr(), y_pred.data_ptr(), n_seq, n_steps, int(num_classes),
                                          float(overlap), int(ignore_value) if ignore_value is not None else 0,
                                          int(ignore_value is not None), scratch.data_ptr(), f1.data_ptr(),
                                          valid.data_ptr(), self._stream()), 'twog_f1_at_k')
        return f1, valid

    def eval_limits(self):
        """(largest class count of eval_update / confusion_counts, positions one trip of their capped grid covers)."""
        max_classes, per_trip = C.c_int(0), C.c_int(0)
        self._check(self.lib.twog_eval_limits(C.byref(max_classes), C.byref(per_trip)), 'twog_eval_limits')
        return max_classes.value, per_trip.value

    def eval_update(self, logp, downsampling, target, step_index, counts, flags, want_labels=False):
        """One pass over one (bs, C, T, E) output: ADDS the (true, predicted) pairs of the evaluated positions to counts
        int64 (C, C) and the two error counters to flags int64 (2,), in place. target int64 (bs, T_tgt, E), -1 ignored;
        step_index int32 (bs, S) or None. With want_labels returns (labels, targets) int64 (bs, S or T_tgt, E)."""
        assert logp.dim() == 4 and logp.dtype == torch.float32
        assert target.dim() == 3 and target.dtype == torch.int64 and target.shape[0] == logp.shape[0] \
            and target.shape[2] == logp.shape[3], (tuple(target.shape), tuple(logp.shape))
        logp, target = logp.contiguous(), target.contiguous()
        bs, Cn, T, E = logp.shape
        T_tgt = target.shape[1]
        assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() == Cn * Cn
        assert flags.dtype == torch.int64 and flags.is_contiguous() and flags.numel() == 2
        S = T_tgt
        if step_index is not None:
            assert step_index.dim() == 2 and step_index.dtype == torch.int32 and step_index.shape[0] == bs
            step_index = step_index.contiguous()
            S = step_index.shape[1]
        labels = targets = None
        if want_labels:
            labels = torch.empty(bs, S, E, dtype=torch.int64, device=logp.device)
            targets = torch.empty(bs, S, E, dtype=torch.int64, device=logp.device)
        self._check(self.lib.twog_eval_update(logp.data_ptr(), bs, Cn, T, E, int(downsampling), target.data_ptr(), T_tgt,
                                              _ptr(step_index), S, counts.data_ptr(), flags.data_ptr(), _ptr(labels),
                                              _ptr(targets), self._stream()), 'twog_eval_update')
        return (labels, targets) if want_labels else None

    def confusion_counts(self, y_true, y_pred, num_classes, counts, flags):
        """ADDS the (true, predicted) pairs of two int64 label tensors of equal size to counts int64 (C, C), in place;
        true == -1 is ignored, any other label outside [0, C) is counted in flags[0]."""
        y_true, y_pred = y_true.to(torch.int64).contiguous(), y_pred.to(torch.int64).contiguous()
        assert y_true.numel() == y_pred.numel()
        assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() == num_classes * num_classes
        assert flags.dtype == torch.int64 and flags.is_contiguous() and flags.numel() == 2
        self._check(self.lib.twog_confusion_counts(y_true.data_ptr(), y_pred.data_ptr(), y_true.numel(), int(num_classes),
                                                   counts.data_ptr(), flags.data_ptr(), self._stream()),
                    'twog_confusion_counts')
        return counts

    def class_counts(self, targets, num_classes, ignore_index, counts):
        """ADDS the number of labels of each class in an int64 tensor to counts int64 (C,), in place, under the NLL term's
        rule: a label equal to ignore_index or outside [0, C) is skipped."""
        assert targets.dtype == torch.int64 and targets.is_contiguous()
        assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() == num_classes
        assert counts.device == targets.device
        self._check(self.lib.twog_class_counts(targets.data_ptr(), targets.numel(), int(num_classes), int(ignore_index),
                                               counts.data_ptr(), self._stream()), 'twog_class_counts')
        return counts

    def segment_f1_limits(self):
        """(longest sequence segment_f1 takes, most overlaps of one call)."""
        max_steps, max_overlaps = C.c_int(0), C.c_int(0)
        self._check(self.lib.twog_segment_f1_limits(C.byref(max_steps), C.byref(max_overlaps)), 'twog_segment_f1_limits')
        return max_steps.value, max_overlaps.value

    def segment_f1(self, y_true, y_pred, num_classes, overlaps, ignore_value=None, entity_minor=False):
        """Per-sequence segmental F1@k for every overlap from one matching, one launch. int64 labels, read in place:
        (n_seq, n_steps), or with entity_minor (bs, n_steps, E) as eval_update writes them (sequence b * E + e). Returns
        (f1 float64 (n_seq, K), tp, fp, fn int32 (n_seq, K), valid int32 (n_seq,), packed): the five are views of the one
        int64 buffer `packed`, so that a caller who wants them on the host makes one copy (see unpack_segment_f1)."""
        assert y_true.dtype == torch.int64 and y_pred.dtype == torch.int64 and y_true.shape == y_pred.shape
        assert y_true.dim() == (3 if entity_minor else 2), tuple(y_true.shape)
        y_true, y_pred = y_true.contiguous(), y_pred.contiguous()
        if entity_minor:
            bs, n_steps, E = y_true.shape
            n_seq = bs * E
        else:
            (n_seq, n_steps), E = y_true.shape, 0
        K = len(overlaps)
        ov = (C.c_double * max(K, 1))(*[float(o) for o in overlaps])
        packed = torch.empty(segment_f1_words(n_seq, K), dtype=torch.int64, device=y_true.device)
        f1, tp, fp, fn, valid = unpack_segment_f1(packed, n_seq, K)
        self._check(self.lib.twog_segment_f1(y_true.data_ptr(), y_pred.data_ptr(), n_seq, n_steps, E, int(num_classes), ov, K,
                                             int(ignore_value) if ignore_value is not None else 0,
                                             int(ignore_value is not None), tp.data_ptr(), fp.data_ptr(), fn.data_ptr(),
                                             f1.data_ptr(), valid.data_ptr(), self._stream()), 'twog_segment_f1')
        return f1, tp, fp, fn, valid, packed

    def segment_f1_accumulate(self, f1, valid, f1_sums, valid_sums):
        """f1_sums[k] += f1[:, k].sum(), valid_sums[k] += valid.sum() in fp64 on the device, in a fixed order, in place."""
        n_seq, K = f1.shape
        assert f1.dtype == torch.float64 and f1.is_contiguous() and valid.dtype == torch.int32 and valid.numel() == n_seq
        for t in (f1_sums, valid_sums):
            assert t.dtype == torch.float64 and t.is_contiguous() and t.numel() == K
        self._check(self.lib.twog_segment_f1_accumulate(f1.data_ptr(), valid.data_ptr(), n_seq, K, f1_sums.data_ptr(),
                                                        valid_sums.data_ptr(), self._stream()), 'twog_segment_f1_accumulate')

    def segment_edit_limits(self):
        """The longest sequence segment_edit takes: the max_steps of segment_f1_limits."""
        max_steps = C.c_int(0)
        self._check(self.lib.twog_segment_edit_limits(C.byref(max_steps)), 'twog_segment_edit_limits')
        return max_steps.value

    def segment_edit(self, y_true, y_pred, ignore_value=None, bg_label=None, entity_minor=False):
        """Per-sequence segmental edit score, one launch. int64 labels, read in place in the layouts of segment_f1:
        (n_seq, n_steps), or with entity_minor (bs, n_steps, E). Returns (score float64 (n_seq,), distance, n_true, n_pred,
        valid int32 (n_seq,), packed): the five are views of the one int64 buffer `packed` (see unpack_segment_edit)."""
        assert y_true.dtype == torch.int64 and y_pred.dtype == torch.int64 and y_true.shape == y_pred.shape
        assert y_true.dim() == (3 if entity_minor else 2), tuple(y_true.shape)
        y_true, y_pred = y_true.contiguous(), y_pred.contiguous()
        if entity_minor:
            bs, n_steps, E = y_true.shape
            n_seq = bs * E
        else:
            (n_seq, n_steps), E = y_true.shape, 0
        packed = torch.empty(segment_edit_words(n_seq), dtype=torch.int64, device=y_true.device)
        score, distance, n_true, n_pred, valid = unpack_segment_edit(packed, n_seq)
        self._check(self.lib.twog_segment_edit(y_true.data_ptr(), y_pred.data_ptr(), n_seq, n_steps, E,
                                               int(ignore_value) if ignore_value is not None else 0,
                                               int(ignore_value is not None), int(bg_label) if bg_label is not None else 0,
                                               int(bg_label is not None), score.data_ptr(), distance.data_ptr(),
                                               n_true.data_ptr(), n_pred.data_ptr(), valid.data_ptr(), self._stream()),
                    'twog_segment_edit')
        return score, distance, n_true, n_pred, valid, packed

    # ---------------------------------------------------------------- Viterbi decode under a transition model
    def viterbi_limits(self):
        """(largest class count, most model steps) viterbi_decode takes."""
        max_classes, max_steps = C.c_int(0), C.c_int(0)
        self._check(self.lib.twog_viterbi_limits(C.byref(max_classes), C.byref(max_steps)), 'twog_viterbi_limits')
        return max_classes.value, max_steps.value

    def viterbi_route(self, bs, num_classes, T, E):
        """(route, workspace bytes) of a decode of this shape: 'lds' keeps the back-pointers in LDS, 'workspace' in device
        memory. Launch-free; ValueError beyond viterbi_limits."""
        return L.viterbi_workspace(self.lib, bs, num_classes, T, E)

    def viterbi_decode(self, logp, transitions, initial=None, lengths=None, downsampling=1, target_steps=None):
        """The best label path of every (clip, entity) sequence of (bs, C, T, E) log-probabilities under fp32 (C, C)
        transition scores (row = from) and optional (C,) initial scores, as include/twog_gcn.h defines it at
        twog_viterbi_decode. lengths: int64 (bs,) on the device, in model steps, or None. Returns (labels int64 (bs,
        target_steps, E), upsampled like predict_labels, and score fp32 (bs, E)). ValueError beyond viterbi_limits,
        before any launch."""
        assert logp.dim() == 4 and logp.dtype == torch.float32
        logp = logp.contiguous()
        bs, Cn, T, E = logp.shape
        max_classes, max_steps = self.viterbi_limits()
        if Cn > max_classes or T > max_steps:
            raise ValueError(f'viterbi_decode takes up to {max_classes} classes and {max_steps} model steps, not {Cn} and {T}')
        assert transitions.shape == (Cn, Cn) and transitions.dtype == torch.float32 and transitions.is_contiguous() \
            and transitions.device == logp.device, (tuple(transitions.shape), transitions.dtype)
        if initial is not None:
            assert initial.shape == (Cn,) and initial.dtype == torch.float32 and initial.is_contiguous() \
                and initial.device == logp.device
        if lengths is not None:
            assert lengths.shape == (bs,) and lengths.dtype == torch.int64 and lengths.is_contiguous() \
                and lengths.device == logp.device, (tuple(lengths.shape), lengths.dtype, lengths.device)
        target_steps = T * int(downsampling) if target_steps is None else int(target_steps)
        labels = torch.empty(bs, target_steps, E, dtype=torch.int64, device=logp.device)
        score = torch.empty(bs, E, dtype=torch.float32, device=logp.device)
        if bs == 0 or E == 0 or T == 0:
            return labels, score
        _, ws_bytes = self.viterbi_route(bs, Cn, T, E)
        ws = self.workspace(ws_bytes, logp.device, 'viterbi') if ws_bytes else None
        self._check(self.lib.twog_viterbi_decode(logp.data_ptr(), bs, Cn, T, E, transitions.data_ptr(), _ptr(initial),
                                                 _ptr(lengths), max(1, int(downsampling)), target_steps, labels.data_ptr(),
                                                 score.data_ptr(), _ptr(ws), ws_bytes, self._stream()), 'twog_viterbi_decode')
        return labels, score

    def transition_counts(self, targets, num_classes, stride, ignore_index, counts):
        """ADDS to counts int64 (C, C) (row = from, column = to) the label pairs (targets[b, k * stride, e], targets[b,
        (k + 1) * stride, e]) of an int64 (bs, T_tgt, E) tensor, in place; a pair with a label equal to ignore_index or
        outside [0, C) is skipped."""
        assert targets.dim() == 3 and targets.dtype == torch.int64 and targets.is_contiguous()
        assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.shape == (num_classes, num_classes)
        assert counts.device == targets.device
        bs, T_tgt, E = targets.shape
        if bs and E:
            self._check(self.lib.twog_transition_counts(targets.data_ptr(), bs, T_tgt, E, int(num_classes), int(stride),
                                                        int(ignore_index), counts.data_ptr(), self._stream()),
                        'twog_transition_counts')
        return counts

    # ---------------------------------------------------------------- segmental decode under a duration model
    def segdecode_limits(self):
        """(largest class count, most model steps, longest duration) segment_decode takes."""
        max_classes, max_steps, max_duration = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.lib.twog_segdecode_limits(C.byref(max_classes), C.byref(max_steps), C.byref(max_duration)),
                    'twog_segdecode_limits')
        return max_classes.value, max_steps.value, max_duration.value

    def segdecode_plan(self, bs, num_classes, T, E, D):
        """The launch of a segmental decode of this shape as a dict: class_template, waves per workgroup, groups per clip,
        route ('lds' keeps the back-pointers in LDS, 'workspace' in device memory) and workspace_bytes. Launch-free;
        ValueError beyond segdecode_limits."""
        return L.segdecode_plan(self.lib, bs, num_classes, T, E, D)

    def segment_decode(self, logp, transitions, durations, initial=None, lengths=None, downsampling=1, target_steps=None):
        """The best segmentation of every (clip, entity) sequence of (bs, C, T, E) log-probabilities under fp32 (C, C)
        segment-transition scores (row = from), fp32 (C, D) duration scores (column l - 1: a segment of l steps) and
        optional (C,) initial scores, as include/twog_gcn.h defines it at twog_segdecode. lengths: int64 (bs,) on the
        device, in model steps, or None. Returns (labels int64 (bs, target_steps, E), upsampled like predict_labels, and
        score fp32 (bs, E)). ValueError beyond segdecode_limits, before any launch."""
        assert logp.dim() == 4 and logp.dtype == torch.float32
        logp = logp.contiguous()
        bs, Cn, T, E = logp.shape
        assert durations.dim() == 2 and durations.shape[0] == Cn and durations.shape[1] >= 1 \
            and durations.dtype == torch.float32 and durations.is_contiguous() and durations.device == logp.device, \
            (tuple(durations.shape), durations.dtype)
        D = durations.shape[1]
        max_classes, max_steps, max_duration = self.segdecode_limits()
        if Cn > max_classes or T > max_steps or D > max_duration:
            raise ValueError(f'segment_decode takes up to {max_classes} classes, {max_steps} model steps and durations up to '
                             f'{max_duration}, not {Cn}, {T} and {D}')
        assert transitions.shape == (Cn, Cn) and transitions.dtype == torch.float32 and transitions.is_contiguous() \
            and transitions.device == logp.device, (tuple(transitions.shape), transitions.dtype)
        if initial is not None:
            assert initial.shape == (Cn,) and initial.dtype == torch.float32 and initial.is_contiguous() \
                and initial.device == logp.device
        if lengths is not None:
            assert lengths.shape == (bs,) and lengths.dtype == torch.int64 and lengths.is_contiguous() \
                and lengths.device == logp.device, (tuple(lengths.shape), lengths.dtype, lengths.device)
        target_steps = T * int(downsampling) if target_steps is None else int(target_steps)
        labels = torch.empty(bs, target_steps, E, dtype=torch.int64, device=logp.device)
        score = torch.empty(bs, E, dtype=torch.float32, device=logp.device)
        if bs == 0 or E == 0 or T == 0:
            return labels, score
        ws_bytes = self.segdecode_plan(bs, Cn, T, E, D)['workspace_bytes']
        ws = self.workspace(ws_bytes, logp.device, 'segdecode') if ws_bytes else None
        self._check(self.lib.twog_segdecode(logp.data_ptr(), bs, Cn, T, E, transitions.data_ptr(), _ptr(initial),
                                            durations.data_ptr(), D, _ptr(lengths), max(1, int(downsampling)), target_steps,
                                            labels.data_ptr(), score.data_ptr(), _ptr(ws), ws_bytes, self._stream()),
                    'twog_segdecode')
        return labels, score

    def duration_counts(self, targets, num_classes, max_duration, stride, ignore_index, counts):
        """ADDS to counts int64 (C, D) the maximal runs of equal labels of an int64 (bs, T_tgt, E) tensor read at every
        `stride`-th step, in place: a run of n labels c adds one to counts[c, min(n, D) - 1]; a label equal to ignore_index
        or outside [0, C) ends a run and starts none."""
        assert targets.dim() == 3 and targets.dtype == torch.int64 and targets.is_contiguous()
        assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.shape == (num_classes, max_duration)
        assert counts.device == targets.device
        bs, T_tgt, E = targets.shape
        if bs and E:
            self._check(self.lib.twog_duration_counts(targets.data_ptr(), bs, T_tgt, E, int(num_classes), int(max_duration),
                                                      int(stride), int(ignore_index), counts.data_ptr(), self._stream()),
                        'twog_duration_counts')
        return counts


def viterbi_decode(logp, transitions, initial=None, lengths=None, downsampling=1, target_steps=None):
    """`get_kernels().viterbi_decode`: see HipKernels.viterbi_decode."""
    return get_kernels().viterbi_decode(logp, transitions, initial, lengths, downsampling, target_steps)


def viterbi_limits():
    """`get_kernels().viterbi_limits()`: (largest class count, most model steps)."""
    return get_kernels().viterbi_limits()


def crf_limits():
    """`get_kernels().crf_limits()`: (largest class count, most model steps) of the CRF loss."""
    return get_kernels().crf_limits()


def transition_counts(targets, num_classes, stride, ignore_index, counts):
    """`get_kernels().transition_counts`: see HipKernels.transition_counts."""
    return get_kernels().transition_counts(targets, num_classes, stride, ignore_index, counts)


def segment_decode(logp, transitions, durations, initial=None, lengths=None, downsampling=1, target_steps=None):
    """`get_kernels().segment_decode`: see HipKernels.segment_decode."""
    return get_kernels().segment_decode(logp, transitions, durations, initial, lengths, downsampling, target_steps)


def segdecode_limits():
    """`get_kernels().segdecode_limits()`: (largest class count, most model steps, longest duration)."""
    return get_kernels().segdecode_limits()


def segdecode_plan(bs, num_classes, T, E, D):
    """`get_kernels().segdecode_plan`: see HipKernels.segdecode_plan."""
    return get_kernels().segdecode_plan(bs, num_classes, T, E, D)


def semicrf_limits():
    """`get_kernels().semicrf_limits()`: (largest class count, most model steps, longest duration) of the semi-Markov CRF loss."""
    return get_kernels().semicrf_limits()


def semicrf_plan(bs, num_classes, T, E, D):
    """`get_kernels().semicrf_plan`: see HipKernels.semicrf_plan."""
    return get_kernels().semicrf_plan(bs, num_classes, T, E, D)


def duration_counts(targets, num_classes, max_duration, stride, ignore_index, counts):
    """`get_kernels().duration_counts`: see HipKernels.duration_counts."""
    return get_kernels().duration_counts(targets, num_classes, max_duration, stride, ignore_index, counts)


def segment_f1_words(n_seq, K):
    """8-byte words of the packed result of segment_f1: n_seq * K fp64, then (3 * n_seq * K + n_seq) int32."""
    return n_seq * K + (3 * n_seq * K + n_seq + 1) // 2


def unpack_segment_f1(packed, n_seq, K):
    """(f1, tp, fp, fn, valid) as views of the packed int64 buffer of segment_f1, on whichever device it is."""
    f1 = packed[:n_seq * K].view(torch.float64).view(n_seq, K)
    ints = packed[n_seq * K:].view(torch.int32)
    tp, fp, fn = (ints[j * n_seq * K:(j + 1) * n_seq * K].view(n_seq, K) for j in range(3))
    return f1, tp, fp, fn, ints[3 * n_seq * K:3 * n_seq * K + n_seq]


def segment_edit_words(n_seq):
    """8-byte words of the packed result of segment_edit: n_seq fp64, then 4 * n_seq int32."""
    return 3 * n_seq


def unpack_segment_edit(packed, n_seq):
    """(score, distance, n_true, n_pred, valid) as views of the packed int64 buffer of segment_edit, on whichever device
    it is."""
    score = packed[:n_seq].view(torch.float64)
    ints = packed[n_seq:3 * n_seq].view(torch.int32)
    distance, n_true, n_pred, valid = (ints[j * n_seq:(j + 1) * n_seq] for j in range(4))
    return score, distance, n_true, n_pred, valid


_backend = None


def get_kernels():
    """The process-wide kernel backend. Always the HIP library; raises if it is not built."""
    global _backend
    if _backend is None:
        _backend = HipKernels()
    return _backend


def _set_backend_for_tests(backend):
    """Test hook: tests/ inject a torch implementation of this interface to exercise the host logic without a GPU.
    Never called from the product path."""
    global _backend
    _backend = backend
