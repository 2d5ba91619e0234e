"""Shared by tests/test_matmul_precision_gpu.py and tools/matmul_precision_cost.py: the GEMM cases of the reduced matmul
precisions against the specification (tests/matmul_precision_ref.py), the same-sign cases, and the small full model whose
projections take the 128x128 class under TWOG_GEMM_TILE=128. Run as a program it is the child process of the full-model
test and the writer of the two records:

    python tests/matmul_precision_cases.py model SEED [SEED ...]     one 'RES {json}' line (needs TWOG_GEMM_TILE=128)
    python tests/matmul_precision_cases.py record-gemm OUT.json      profiles/matmul_precision_gemm.json
    python tests/matmul_precision_cases.py record-model OUT.json     profiles/matmul_precision_model.json (seeds 0..7)
"""
import contextlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import matmul_precision_ref as R  # noqa: E402

DEV = 'cuda:0'
MODES = ('high', 'medium')
C_MODE = {'high': R.C_HIGH, 'medium': R.C_MEDIUM}


# ---- the specification's roundings on the device (int32 arithmetic wraps like the uint32 arithmetic of the numpy functions;
# finite operands only). check_port() holds them against the numpy functions, bit for bit, on the head of every operand.
def t_round_medium(x):
    u = x.contiguous().view(torch.int32)
    return ((u + 0x7fff + ((u >> 16) & 1)) & -65536).view(torch.float32)


def t_split_high(x):
    h = t_round_medium(x)
    return h, t_round_medium(x.contiguous() - h)


def check_port(x, n=1 << 18):
    s = x.contiguous().view(-1)[:n]
    h, m = t_split_high(s)
    hn, mn = R.split_high(s.cpu().numpy())
    assert np.array_equal(h.cpu().numpy().view(np.uint32), hn.view(np.uint32))
    assert np.array_equal(m.cpu().numpy().view(np.uint32), mn.view(np.uint32))


def precision(K, mode):
    """None: no call at all (the default path)."""
    return contextlib.nullcontext() if mode is None else K.matmul_precision(mode)


def p_bits(K, mode):
    return {None: 0, 'highest': 0, 'high': K.GEMM_P3, 'medium': K.GEMM_P1}[mode]


# name: (M, N, K, a_kmajor, b_kmajor, epilogue / layout flags) -- shapes that take the 128x128 class by themselves
GEMM_CASES = {
    'NN bias relu': (4096, 1536, 512, False, False, dict(bias=True, act=1)),
    'NT accumulate': (4096, 512, 1536, False, True, dict(acc=True)),
    'TT splitk': (1536, 512, 16384, True, True, dict()),
    'TN': (1024, 2048, 1024, True, False, dict()),
    'TT grouped rows': (1536, 512, 8192, True, True, dict(grouped=True)),
}
OPERANDS = ('signed', 'wide')   # wide: A spread over +-30 decades with exact zeros and a denormal


class GemmCase:
    """Operands of one case on the device, the launch in a given mode, and the fp64 references."""

    def __init__(self, K, name, kind, seed=7, same_sign=False, shape=None):
        self.K = K
        M, N, Kk, akm, bkm, fl = shape if shape is not None else GEMM_CASES[name]
        self.M, self.N, self.Kk, self.akm, self.bkm = M, N, Kk, akm, bkm
        self.act, self.acc, self.grouped = fl.get('act', 0), fl.get('acc', False), fl.get('grouped', False)
        g = torch.Generator().manual_seed(seed)
        rows_a = Kk // 4 * 5 if self.grouped else Kk   # grouped: all but the first of every 5 stored rows
        A = torch.randn((rows_a, M) if akm else (M, Kk), generator=g)
        if kind == 'wide':
            A = A * 10.0 ** torch.randint(-30, 30, A.shape, generator=g).float()
            A.view(-1)[::97] = 0.0
            A.view(-1)[5 + (M if self.grouped else 0)] = 1e-39
        B = torch.randn((Kk, N) if bkm else (N, Kk), generator=g) * 0.1
        if same_sign:   # post-ReLU activations x non-negative values: every product >= 0
            A, B = torch.relu(A), B.abs()
        self.A, self.B = A.to(DEV), B.to(DEV)
        self.bias = torch.randn(N, generator=g).to(DEV) if fl.get('bias') else None
        self.C0 = torch.randn(M, N, generator=g).to(DEV)
        check_port(self.A)
        check_port(self.B)

    def view_a(self, store):
        return store.view(self.Kk // 4, 5, self.M)[:, 1:, :] if self.grouped else store

    def launch(self, mode, A=None, B=None):
        """-> (C, class bits). mode None: no precision call."""
        A = self.A if A is None else A
        B = self.B if B is None else B
        C = self.C0.clone()
        with precision(self.K, mode):
            self.K.gemm([dict(A=self.view_a(A), B=B, C=C, bias=self.bias, act=self.act, accumulate=self.acc)],
                        a_kmajor=self.akm, b_kmajor=self.bkm)
            cls = self.K.gemm_last_class()
        return C, cls

    def logical(self, A, B):
        """fp64 (M, K) and (K, N)."""
        A = self.view_a(A)
        Ad = (A.reshape(-1, self.M).t() if self.akm else A).double()
        return Ad, (B.double() if self.bkm else B.double().t())

    def epilogue(self, prod):
        if self.bias is not None:
            prod = prod + self.bias.double()
        if self.acc:
            prod = prod + self.C0.double()
        return torch.relu(prod) if self.act else prod

    def planes(self, mode):
        """The spec-rounded operands of `mode`: ((A_h, A_m or None), (B_h, B_m or None)), stored like A and B."""
        if mode == 'medium':
            return (t_round_medium(self.A), None), (t_round_medium(self.B), None)
        return t_split_high(self.A), t_split_high(self.B)

    def kept_ref(self, mode):
        """fp64 sum of the kept products of the spec-rounded operands, through the epilogue."""
        (ah, am), (bh, bm) = self.planes(mode)
        Ah, Bh = self.logical(ah, bh)
        prod = Ah @ Bh
        if mode == 'high':
            Am, Bm = self.logical(am, bm)
            prod = prod + Ah @ Bm + Am @ Bh
        return self.epilogue(prod)

    def rounded_sum(self, mode):
        """The rounded operands as single fp32 tensors: h ('medium') or h + m ('high': exact in fp32)."""
        (ah, am), (bh, bm) = self.planes(mode)
        return (ah, bh) if mode == 'medium' else (ah + am, bh + bm)


def gemm_case_figures(K, name, kind, same_sign=False, shape=None):
    """Runs one case in the three modes and returns the figures the test asserts on (and prints)."""
    c = GemmCase(K, name, kind, same_sign=same_sign, shape=shape)
    X3T = K.GEMM_X3 | K.GEMM_TILE128
    out = dict(case=name, operands='same-sign' if same_sign else kind, M=c.M, N=c.N, K=c.Kk, modes={})
    A64, B64 = c.logical(c.A, c.B)
    ref = c.epilogue(A64 @ B64)
    absum = A64.abs() @ B64.abs()
    Ch, cls = c.launch(None)
    out['class_default'] = cls
    out['default_ok'] = bool((cls & X3T) == X3T and not cls & (K.GEMM_P3 | K.GEMM_P1))
    Ch2, cls2 = c.launch('highest')
    out['highest_bit_identical_to_default'] = bool(torch.equal(Ch, Ch2) and cls2 == cls)
    e_abs = float((Ch.double() - ref).abs().max())
    out['highest_err_of_largest'] = e_abs / float(ref.abs().max())
    if same_sign:
        out['highest_mean_signed_rel_err'] = float(((Ch.double() - ref) / ref.clamp_min(1e-300)).mean())
    for mode in MODES:
        C1, cls1 = c.launch(mode)
        C2, _ = c.launch(mode)
        f = dict(cls=cls1)
        f['class_ok'] = bool((cls1 & X3T) == X3T and (cls1 & (K.GEMM_P3 | K.GEMM_P1)) == p_bits(K, mode)
                             and (cls1 & ~(K.GEMM_P3 | K.GEMM_P1)) == cls)
        f['bit_identical'] = bool(torch.equal(C1, C2))
        # (c) against the kept products of the spec-rounded operands; the 'highest' kernel on those same rounded operands
        kept = c.kept_ref(mode)
        f['err_vs_kept_of_largest'] = float((C1.double() - kept).abs().max() / kept.abs().max())
        Ar, Br = c.rounded_sum(mode)
        Cr, _ = c.launch(None, Ar, Br)
        Ar64, Br64 = c.logical(Ar, Br)
        ref_r = c.epilogue(Ar64 @ Br64)
        f['highest_on_rounded_err_of_largest'] = float((Cr.double() - ref_r).abs().max() / ref_r.abs().max())
        # (d) against the unrounded fp64 product, per element
        excess = (C1.double() - ref).abs() - (C_MODE[mode] * absum + e_abs)
        f['bound_excess_max'] = float(excess.max())
        f['err_over_sum_abs_max'] = float(((C1.double() - ref).abs() / absum.clamp_min(1e-300)).max())
        f['differs_from_highest'] = bool(not torch.equal(C1, Ch))
        if same_sign:
            f['mean_signed_rel_err'] = float(((C1.double() - ref) / ref.clamp_min(1e-300)).mean())
        out['modes'][mode] = f
        del kept, Ar, Br, Cr, Ar64, Br64, ref_r, excess
    return out


# same-sign operands (post-ReLU x non-negative), TT; K = 1 536 needs 384 tiles to take the class by itself
SAME_SIGN_CASES = {'same-sign TT K=1536': (4096, 1536, 1536, True, True, dict()),
                   'same-sign TT K=16384': (1536, 512, 16384, True, True, dict())}


# ---------------------------------------------------------------------------------------------------------------- full model
MODEL_SHAPE = dict(bs=2, T=6, H=2, O=3, N=19, h=128)


def model_run(seeds):
    """The small model with the segmentation given for humans and objects (no learned hard gate), projections forced onto
    the 128x128 class by TWOG_GEMM_TILE=128 in the environment. Per seed: one eval forward and one train forward + backward
    in each precision; the class bits of every HipKernels.gemm launch are collected by a wrapper. Returns per seed the
    deviations from 'highest' and the checks."""
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd import kernels
    from twog_gcn_amd.models import TGGCN
    assert os.environ.get('TWOG_GEMM_TILE') == '128'
    K = kernels.get_kernels()
    assert K.name == 'hip'
    s = MODEL_SHAPE
    bs, T, H, O, N, h = s['bs'], s['T'], s['H'], s['O'], s['N'], s['h']
    cfg = dict(hidden_size=h, gcn_node=N, attention_style='v3', discrete_optimization_strategy='gs', message_segment=True,
               message_type='v2', message_granularity='v1', message_aggregation='att', object_segment_update_strategy='ind')
    seen = []
    real_gemm = type(K).gemm

    def counting_gemm(self, problems, *a, **kw):
        real_gemm(self, problems, *a, **kw)
        if problems and not kw.get('chain') and self._tape is None:
            seen.append(self.gemm_last_class())
    type(K).gemm = counting_gemm
    res = {}
    try:
        for seed in seeds:
            torch.manual_seed(seed)
            m0 = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(13, None), **cfg)
            sd = {k: v.detach().clone() for k, v in m0.state_dict().items()}
            g = torch.Generator().manual_seed(1000 + seed)
            x_human = torch.cat([torch.relu(torch.randn(bs, T, H, 2048, generator=g)), torch.rand(bs, T, H, 4 * N, generator=g)], -1).to(DEV)
            x_objects = torch.relu(torch.randn(bs, T, O, 2048, generator=g)).to(DEV)
            mask = torch.ones(bs, O, device=DEV)
            seg_h = (torch.rand(bs, T, H, generator=g) < 0.4).float().to(DEV)
            seg_o = (torch.rand(bs, T, O, generator=g) < 0.4).float().to(DEV)
            cot = []   # cotangents of the four log-probability outputs, drawn once per seed (first run)

            def run(mode, call):
                m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(13, None), **cfg)
                m.load_state_dict(sd)
                m = m.to(DEV)
                if call:
                    assert m.use_matmul_precision(mode) is m
                r = dict(bits_fwd=0, bits_bwd=0)
                m.eval()
                with torch.no_grad():
                    r['eval'] = [o.detach().clone() for o in m(x_human, x_objects, mask, human_segmentation=seg_h,
                                                               objects_segmentation=seg_o)]
                m.train()
                del seen[:]
                out = m(x_human, x_objects, mask, human_segmentation=seg_h, objects_segmentation=seg_o)
                for c_ in seen:
                    r['bits_fwd'] |= c_
                del seen[:]
                if not cot:
                    cot.extend(torch.randn(o.shape, generator=g).to(DEV) for o in out[2:6])
                sum((o * c_).sum() for o, c_ in zip(out[2:6], cot)).backward()
                torch.cuda.synchronize()
                for c_ in seen:
                    r['bits_bwd'] |= c_
                r['train'] = [o.detach().clone() for o in out]
                r['grads'] = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
                r['precision_after'] = K.lib.twog_gemm_get_precision()
                return r

            base = run('highest', call=False)
            again = run('highest', call=True)
            P = K.GEMM_P3 | K.GEMM_P1
            X3T = K.GEMM_X3 | K.GEMM_TILE128
            one = dict(
                highest_identical=bool(all(torch.equal(a, b) for k in ('eval', 'train') for a, b in zip(base[k], again[k]))
                                       and all(torch.equal(base['grads'][n], again['grads'][n]) for n in base['grads'])),
                highest_takes_the_class=bool((base['bits_fwd'] & X3T) == X3T and (base['bits_bwd'] & X3T) == X3T),
                highest_p_bits=int((base['bits_fwd'] | base['bits_bwd'] | again['bits_fwd'] | again['bits_bwd']) & P),
                n_grads=len(base['grads']), modes={})
            for mode in MODES:
                r = run(mode, call=True)
                finite = all(bool(torch.isfinite(o).all()) for k in ('eval', 'train') for o in r[k]) and \
                    all(bool(torch.isfinite(v).all()) for v in r['grads'].values())
                dev_out = max(float((a - b).abs().max()) for k in ('eval', 'train') for a, b in zip(r[k][2:6], base[k][2:6]))
                dev_grad, worst = 0.0, None
                for n, gb in base['grads'].items():
                    d = float((r['grads'][n] - gb).abs().max() / gb.abs().max().clamp_min(1e-30))
                    if d > dev_grad:
                        dev_grad, worst = d, n
                one['modes'][mode] = dict(finite=bool(finite), p_bits_fwd=int(r['bits_fwd'] & P), p_bits_bwd=int(r['bits_bwd'] & P),
                                          want=p_bits(K, mode), same_grad_names=bool(r['grads'].keys() == base['grads'].keys()),
                                          out_max_abs=dev_out, grad_of_scale=dev_grad, worst_grad=worst,
                                          precision_after=int(r['precision_after']))
            res[str(seed)] = one
    finally:
        type(K).gemm = real_gemm
    return res


def main(argv):
    what = argv[0]
    if what == 'model':
        print('RES ' + json.dumps(model_run([int(a) for a in argv[1:]])), flush=True)
        return
    if what == 'record-model':
        res = model_run(list(range(8)))
        rec = dict(device=torch.cuda.get_device_name(0), shape=MODEL_SHAPE, TWOG_GEMM_TILE=128,
                   what="deviation of 'high' / 'medium' from 'highest' (same weights and inputs): outputs = max abs over the four "
                        "log-probability outputs of an eval and a train forward, gradients = max abs over the tensor's max abs, "
                        "worst tensor",
                   seeds=res,
                   worst={mode: dict(out_max_abs=max(v['modes'][mode]['out_max_abs'] for v in res.values()),
                                     grad_of_scale=max(v['modes'][mode]['grad_of_scale'] for v in res.values())) for mode in MODES})
    else:
        assert what == 'record-gemm', what
        import twog_gcn_amd  # noqa: F401
        from twog_gcn_amd import kernels
        K = kernels.get_kernels()
        rows = [gemm_case_figures(K, name, kind) for name in GEMM_CASES for kind in OPERANDS]
        rows += [gemm_case_figures(K, name, 'signed', same_sign=True, shape=shape) for name, shape in SAME_SIGN_CASES.items()]
        rec = dict(device=torch.cuda.get_device_name(0), C_HIGH=R.C_HIGH, C_MEDIUM=R.C_MEDIUM,
                   existing_same_sign_bias_caps_of_highest={'64': 1e-7, '128': 1.0e-6, '128 K=61440': 3.0e-6},   # tests/test_kernels_gpu.py
                   what='per case and mode: error against the fp64 kept products of the spec-rounded operands (of the largest '
                        "output), the 'highest' kernel's error on those rounded operands, the worst |error| / sum|a||b| against "
                        'the unrounded fp64 product, and on same-sign operands the mean signed relative error',
                   cases=rows)
    with open(argv[1], 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec.get('worst', {r['case'] + ' / ' + r['operands']: {m: v.get('mean_signed_rel_err', v['err_over_sum_abs_max'])
                                                                           for m, v in r['modes'].items()}
                                       for r in rec.get('cases', [])})))


if __name__ == '__main__':
    main(sys.argv[1:])
