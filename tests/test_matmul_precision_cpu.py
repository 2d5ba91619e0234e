"""Opt-in matmul precision ('high' / 'medium' of the bf16x3 128x128 GEMM class), without a GPU: the properties and error
constants of the numpy specification (tests/matmul_precision_ref.py) and the host layer of ops.py / models.py on the test
double (tests/matmul_precision_fake.py)."""
import copy

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from tests import matmul_precision_ref as R
from tests.fake_kernels import FakeKernels
from tests.helpers import g4_inputs, load_g4
from tests.input_grad_cases import build_model
from tests.matmul_precision_fake import MatmulPrecisionFakeKernels

CASE = 'c2_stage1'
MAXN = np.float32(3.3895314e38)   # the largest bf16; its fp32 neighbours round to it (below 0x7f7f8000: no overflow to Inf)


def _values(seed=0, n=200_000):
    """Seeded fp32 values over 60 decades, both signs, with exact zeros, a denormal and the neighbours of +-max-normal bf16."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)).astype(np.float32)
    edge = np.array([0.0, -0.0, 1e-39, -1e-39, MAXN, -MAXN, np.nextafter(MAXN, np.float32(0)), -np.nextafter(MAXN, np.float32(0)),
                     np.nextafter(MAXN, np.float32(np.inf)), -np.nextafter(MAXN, np.float32(np.inf)), 1.0, 1.0 + 2.0 ** -8,
                     1.0 + 3 * 2.0 ** -8, 2.0 - 2.0 ** -23], dtype=np.float32)
    return np.concatenate([edge, x])


def _is_bf16(v):
    return bool(((v.view(np.uint32) & 0xffff) == 0).all())


# ---------------------------------------------------------------------------------------------------------------- spec
def test_planes_are_bf16_and_h_plus_m_is_exact():
    x = _values()
    h, m = R.split_high(x)
    r = R.round_medium(x)
    assert h.dtype == m.dtype == r.dtype == np.float32
    assert _is_bf16(h) and _is_bf16(m) and _is_bf16(r)
    assert np.array_equal(h, r)   # the 'high' h plane IS the 'medium' plane
    assert np.isfinite(h).all() and np.isfinite(m).all()
    s32 = h + m                                              # fp32 add
    s64 = h.astype(np.float64) + m.astype(np.float64)        # exact
    assert np.array_equal(s32.astype(np.float64), s64)


def test_per_operand_bounds():
    x = _values(1)
    x64 = x.astype(np.float64)
    h, m = R.split_high(x)
    e_high = np.abs(x64 - h.astype(np.float64) - m.astype(np.float64))
    e_med = np.abs(x64 - R.round_medium(x).astype(np.float64))
    assert (e_high <= R.E_HIGH * np.abs(x64) + R.U).all(), float((e_high / np.abs(x64).clip(1e-300)).max())
    assert (e_med <= R.E_MEDIUM * np.abs(x64) + R.U).all(), float((e_med / np.abs(x64).clip(1e-300)).max())
    assert (np.abs(m.astype(np.float64)) <= 2.0 ** -8 * np.abs(x64) + R.U).all()
    # ... and the bounds are not idle: the worst relative errors of a million values come within a factor 2 of them
    big = np.abs(x64) > 1e-30
    assert (e_med[big] / np.abs(x64[big])).max() > R.E_MEDIUM / 2
    assert (e_high[big] / np.abs(x64[big])).max() > R.E_HIGH / 2


def test_ties_go_to_even_and_edges():
    f = lambda *v: np.array(v, dtype=np.float32)
    assert np.array_equal(R.round_medium(f(1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8)), f(1.0, 1.0 + 2.0 ** -6))   # ties: to even
    assert np.array_equal(R.round_medium(f(2.0 - 2.0 ** -23)), f(2.0))                                        # up into the next binade
    z = R.round_medium(f(0.0, -0.0))
    assert np.array_equal(z.view(np.uint32), f(0.0, -0.0).view(np.uint32))
    # top of the range: below 0x7f7f8000 stays finite, from there on Inf; 'high' then has m = -Inf (h + m = NaN)
    top = np.array([0x7f7f7fff, 0x7f7f8000, 0x7f7fffff, 0xff7f8000], dtype=np.uint32).view(np.float32)
    assert np.array_equal(R.round_medium(top), f(MAXN, np.inf, np.inf, -np.inf))
    h, m = R.split_high(top[1:2])
    assert np.isinf(h[0]) and np.isinf(m[0]) and m[0] < 0
    # Inf and NaN
    assert np.array_equal(R.round_medium(f(np.inf, -np.inf)), f(np.inf, -np.inf))
    assert np.isnan(R.round_medium(f(np.nan))).all()
    snan = np.array([0x7f800001], dtype=np.uint32).view(np.float32)   # a NaN whose payload sits in the dropped half
    assert np.isnan(R.round_medium(snan)).all() and _is_bf16(R.round_medium(snan))
    h, m = R.split_high(f(np.inf, np.nan))
    assert np.isnan(m).all()
    # a denormal: rounded on the pattern, absolute error within U
    d = f(1e-39)
    assert abs(float(d[0]) - float(R.round_medium(d)[0])) <= R.U and _is_bf16(R.round_medium(d))


def test_no_bias_on_a_same_sign_sample():
    """Mean signed error of the two roundings on positive values: within 3 standard errors of zero. The sample is uniform on one
    binade, [1, 2): the density is flat over every rounding cell and the two half cells at the ends balance, so a rounding to
    nearest has mean error zero exactly. (A log-uniform sample, or the error relative to x, has a mean of its own of the
    order of the squared spacing: 1 standard error at this sample size.) The truncating split of the 'highest' kernel, put
    through the same check, is hundreds of standard errors off."""
    rng = np.random.default_rng(3)
    x = rng.uniform(1.0, 2.0, 400_000).astype(np.float32)
    x64 = x.astype(np.float64)
    h, m = R.split_high(x)
    for name, err in (('medium', R.round_medium(x).astype(np.float64) - x64),
                      ('high', h.astype(np.float64) + m.astype(np.float64) - x64)):
        se = err.std() / np.sqrt(err.size)
        print(name, 'mean', err.mean(), 'standard error', se)
        assert abs(err.mean()) <= 3 * se, (name, err.mean(), se)
    trunc = (x.view(np.uint32) & 0xffff0000).view(np.float32).astype(np.float64) - x64
    assert abs(trunc.mean()) > 100 * trunc.std() / np.sqrt(trunc.size)   # the check does see a bias where there is one


def test_constants_meet_the_conditions():
    assert R.C_HIGH <= 2.0 ** -13 and R.C_MEDIUM <= 2.0 ** -6
    assert R.C_HIGH >= (2 + 2.0 ** -18) * 2.0 ** -16 and R.C_MEDIUM >= 2.0 ** -7 + 2.0 ** -16   # what the derivation gives


@pytest.mark.parametrize('positive', [False, True])
@pytest.mark.parametrize('K', [16, 512, 2048])
def test_kept_products_stay_within_the_constants(K, positive):
    rng = np.random.default_rng(K + positive)
    M, N = 48, 40
    a = rng.standard_normal((M, K)).astype(np.float32)
    b = (rng.standard_normal((K, N)) * 0.1).astype(np.float32)
    if positive:
        a, b = np.abs(a), np.abs(b)
    else:
        a *= (10.0 ** rng.integers(-6, 6, a.shape)).astype(np.float32)
    exact = a.astype(np.float64) @ b.astype(np.float64)
    absum = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
    slack = 1e-13 * absum   # fp64 rounding of the three K-long sums themselves
    for mode, c in (('high', R.C_HIGH), ('medium', R.C_MEDIUM)):
        err = np.abs(R.kept_products(a, b, mode) - exact)
        ratio = float((err / absum).max())
        print(mode, 'K', K, 'positive', positive, 'worst error / (C sum|a||b|)', ratio / c)
        assert (err <= c * absum + slack).all(), (mode, ratio, c)
    # the two modes are different arithmetic: 'high' is at least 2^5 times closer than 'medium'
    assert np.abs(R.kept_products(a, b, 'high') - exact).max() * 32 < np.abs(R.kept_products(a, b, 'medium') - exact).max()


# ---------------------------------------------------------------------------------------------------------------- host layer
@pytest.fixture()
def fake():
    k = MatmulPrecisionFakeKernels()
    twog_kernels._set_backend_for_tests(k)
    yield k
    twog_kernels._set_backend_for_tests(None)


def _case():
    z, meta = load_g4(CASE)
    return meta, g4_inputs(z)


def _train_step(m, kw):
    """One forward and one backward in training mode with a fixed host seed; returns (outputs, gradients by name)."""
    m.zero_grad()
    torch.manual_seed(11)
    out = m(**kw)
    sum((o * o).sum() for o in out if o.requires_grad).backward()
    return [o.detach().clone() for o in out], {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def test_high_enters_and_leaves_once_per_pass(fake):
    meta, kw = _case()
    m = build_model(meta).train()
    assert m.matmul_precision() == 'highest'
    assert m.use_matmul_precision('high') is m and m.matmul_precision() == 'high'
    torch.manual_seed(11)
    out = m(**kw)
    assert fake.precision_events == [('enter', 'high'), ('exit', 'high')] and fake.precision_depth == 0
    sum((o * o).sum() for o in out if o.requires_grad).backward()
    assert fake.precision_events == [('enter', 'high'), ('exit', 'high')] * 2 and fake.precision_depth == 0
    del fake.precision_events[:]
    m.use_matmul_precision('medium').eval()
    with torch.no_grad():
        m(**kw)
    assert fake.precision_events == [('enter', 'medium'), ('exit', 'medium')]


def test_default_and_highest_never_call_it(fake):
    meta, kw = _case()
    m = build_model(meta).train()
    _train_step(m, kw)
    assert fake.precision_events == []
    m.use_matmul_precision('high')
    assert m.use_matmul_precision('highest') is m and m.matmul_precision() == 'highest'
    _train_step(m, kw)
    assert fake.precision_events == []


def test_unknown_name_state_dict_and_deepcopy(fake):
    meta, kw = _case()
    m = build_model(meta)
    keys = list(m.state_dict().keys())
    for bad in ('tf32', 'HIGH', None, 1):
        with pytest.raises(ValueError):
            m.use_matmul_precision(bad)
    assert m.matmul_precision() == 'highest'
    m.use_matmul_precision('high')
    assert list(m.state_dict().keys()) == keys
    assert 'matmul_precision' not in vars(m)
    assert copy.deepcopy(m).matmul_precision() == 'highest' and m.matmul_precision() == 'high'
    # torch's process-wide setting is never read
    before = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision('medium')
        assert build_model(meta).matmul_precision() == 'highest' and m.matmul_precision() == 'high'
        fresh = build_model(meta).eval()
        with torch.no_grad():
            fresh(**kw)
        assert fake.precision_events == []
    finally:
        torch.set_float32_matmul_precision(before)


def test_a_raising_pass_leaves_the_context(fake):
    meta, kw = _case()
    m = build_model(meta).eval().use_matmul_precision('high')

    def boom(*a, **k):
        raise RuntimeError('boom')
    fake.gemm = boom
    with pytest.raises(RuntimeError, match='boom'), torch.no_grad():
        m(**kw)
    assert fake.precision_events == [('enter', 'high'), ('exit', 'high')] and fake.precision_depth == 0


def test_a_kernels_object_without_the_method_is_tolerated():
    """The plain test double has no matmul_precision: a model set to 'high' runs on it and gives the double's usual results."""
    meta, kw = _case()
    plain = FakeKernels()
    assert not hasattr(plain, 'matmul_precision')
    twog_kernels._set_backend_for_tests(plain)
    try:
        ref = build_model(meta).train()
        m = build_model(meta).train()
        m.load_state_dict(ref.state_dict())
        m.use_matmul_precision('high')
        out_ref, g_ref = _train_step(ref, kw)
        out, g = _train_step(m, kw)
    finally:
        twog_kernels._set_backend_for_tests(None)
    assert len(out) == len(out_ref) and all(torch.equal(a, b) for a, b in zip(out, out_ref))
    assert g.keys() == g_ref.keys() and all(torch.equal(g[n], g_ref[n]) for n in g)
