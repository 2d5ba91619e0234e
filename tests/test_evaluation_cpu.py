"""CPU: the prediction evaluation (confusion counts, precision / recall / F1, the per-class report, the accumulator)
against golden G15 -- the reference's own evaluate_predictions / downsample_bad_bimanual_videos /
summarize_frames_into_segments and scikit-learn 1.7.2, recorded by tools/make_golden_evaluation.py. First the numpy
specification (tests/evaluation_ref.py), then the host layer (2g-gcn_amd/postprocess.py) through the kernel-interface test
double. Integers are compared exactly; every metric within 1e-12 (both sides are fp64 arithmetic on the same integers);
F1@k within 1e-6 of oracle.postprocess_ref.f1_at_k (the per-sequence F1 is stored in fp32)."""
import contextlib
import io
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd import postprocess as pp
from tests import evaluation_ref as E
from tests.evaluation_fake import EvaluationFakeKernels
from tests.helpers import GOLDEN, ROOT
from oracle import postprocess_ref as R

OVERLAPS = (0.1, 0.25, 0.5)
TOL = 1e-12


@pytest.fixture()
def fake_backend():
    twog_kernels._set_backend_for_tests(EvaluationFakeKernels())
    yield
    twog_kernels._set_backend_for_tests(None)


def g15():
    return np.load(f'{GOLDEN}/g15_evaluation.npz')


class Case:
    """One G15 case: heads [(name, C, E, n_names)], batches [[(logp, target) per head]], the step index per batch."""

    def __init__(self, z, name):
        self.z, self.name = z, name
        cfg = [int(v) for v in z[f'{name}_cfg']]
        self.ds, n_batches = cfg[0], cfg[1]
        names = [str(n) for n in z[f'{name}_heads']]
        self.heads = [(n, *cfg[2 + 3 * i:5 + 3 * i]) for i, n in enumerate(names)]
        self.batches = [[(z[f'{name}_b{b}_h{h}_logp'], z[f'{name}_b{b}_h{h}_target']) for h in range(len(names))]
                        for b in range(n_batches)]
        self.step_index = None
        if f'{name}_is_15fps' in z.files:
            self.step_index = pp.half_rate_step_index(self.batches[0][0][1].shape[1], z[f'{name}_is_15fps'])
        if f'{name}_segment_starts' in z.files:
            self.step_index = pp.segment_step_index([[int(s) for s in row if s >= 0] for row in z[f'{name}_segment_starts']])

    def want(self, h, what):
        return self.z[f'{self.name}_h{h}_{what}']


def cases():
    z = g15()
    return [Case(z, str(n)) for n in z['cases']]


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.abs(a - b) <= TOL) | (np.isnan(a) & np.isnan(b))))


def check_metrics(case, h, micro, macro, report):
    """micro / macro {'precision','recall','f1'} and the output_dict report of head h against scikit-learn's."""
    for got, key in ((micro, 'micro'), (macro, 'macro')):
        want = case.want(h, key)
        assert close([got['precision'], got['recall'], got['f1']], want), (case.name, h, key, got, want)
    n_names = case.heads[h][3]
    prefix = 'aff' if 'affordance' in case.heads[h][0] else 'sub'
    row = lambda d: [d['precision'], d['recall'], d['f1-score'], d['support']]
    got_rows = [row(report[f'{prefix}{i}']) for i in range(n_names)]
    assert close(got_rows, case.want(h, 'report_classes')), (case.name, h)
    accuracy = case.want(h, 'report_accuracy')
    if np.isnan(accuracy):
        assert 'accuracy' not in report and close(row(report['micro avg']), case.want(h, 'report_micro')), (case.name, h)
    else:
        assert 'micro avg' not in report and close(report['accuracy'], accuracy), (case.name, h, report.get('accuracy'))
    assert close(row(report['macro avg']), case.want(h, 'report_macro')), (case.name, h, report['macro avg'])
    assert close(row(report['weighted avg']), case.want(h, 'report_weighted')), (case.name, h, report['weighted avg'])
    assert len(report) == n_names + 3


def head_names(case, h):
    prefix = 'aff' if 'affordance' in case.heads[h][0] else 'sub'
    return [f'{prefix}{i}' for i in range(case.heads[h][3])]


def test_golden_covers_the_listed_situations():
    """The fixture really holds the situations the cases were built for (a regenerated fixture cannot lose them)."""
    by_name = {c.name: c for c in cases()}
    plain = by_name['plain'].want(0, 'counts')
    assert plain[4].sum() == 0 and plain[:, 4].sum() > 0          # never true
    assert plain[:, 3].sum() == 0 and plain[3].sum() > 0          # never predicted
    assert plain[2].sum() == 0 and plain[:, 2].sum() == 0         # absent from both
    assert by_name['plain'].want(0, 'labels')[0, 0, 0] == 1       # the tie between classes 1 and 4
    beyond = by_name['beyond_names']
    assert beyond.want(0, 'counts')[:, 4:].sum() > 0 and np.isnan(beyond.want(0, 'report_accuracy'))
    assert by_name['all_ignored'].want(1, 'counts').sum() == 0 and (by_name['all_ignored'].want(1, 'targets') == -1).all()
    assert by_name['all_ignored'].want(1, 'micro')[2] == 0.0 and np.isnan(by_name['all_ignored'].want(1, 'macro')[2])
    assert {(c.ds, c.batches[0][0][1].shape[1] > c.batches[0][0][0].shape[2] * c.ds) for c in by_name.values()} >= \
        {(1, False), (3, False), (4, True)}
    assert {c.heads[0][2] for c in by_name.values()} >= {1, 2}
    assert by_name['bimanual_odd'].batches[0][0][1].shape[1] % 2 == 1 and by_name['bimanual_even'].batches[0][0][1].shape[1] % 2 == 0
    assert by_name['bimanual_odd'].z['bimanual_odd_is_15fps'].sum() == 2
    assert [h[1] for h in by_name['cad120'].heads] == [10, 10, 12, 12]


def test_specification_matches_reference_golden():
    for case in cases():
        for h, (name, C, _, n_names) in enumerate(case.heads):
            counts, flags = np.zeros((C, C), dtype=np.int64), np.zeros(2, dtype=np.int64)
            labels, targets = [], []
            for batch in case.batches:
                logp, tgt = batch[h]
                si = None if case.step_index is None else case.step_index.numpy()
                c, f, lab, kept = E.eval_update(logp, case.ds, tgt, si)
                counts += c
                flags += f
                labels.append(lab)
                targets.append(kept)
            labels, targets = np.concatenate(labels), np.concatenate(targets)
            assert np.array_equal(labels, case.want(h, 'labels')), (case.name, h)
            assert np.array_equal(targets, case.want(h, 'targets')), (case.name, h)
            assert np.array_equal(counts, case.want(h, 'counts')) and not flags.any(), (case.name, h)
            c2, f2 = E.confusion_counts(targets, labels, C)
            assert np.array_equal(c2, counts) and not f2.any()
            check_metrics(case, h, E.precision_recall_f1(counts, 'micro'), E.precision_recall_f1(counts, 'macro'),
                          E.classification_report(counts, head_names(case, h)))


def run_accumulator(case, device, splits=1):
    """The case through EvaluationAccumulator, every batch cut into `splits` parts along the clips."""
    acc = pp.EvaluationAccumulator([h[0] for h in case.heads], [h[1] for h in case.heads], downsampling=case.ds,
                                   overlaps=OVERLAPS)
    for batch in case.batches:
        bs = batch[0][0].shape[0]
        for part in np.array_split(np.arange(bs), min(splits, bs)):
            sl = slice(int(part[0]), int(part[-1]) + 1)
            outs = [torch.from_numpy(lp[sl]).to(device) for lp, _ in batch]
            tgts = [torch.from_numpy(t[sl]).to(device) for _, t in batch]
            si = None if case.step_index is None else case.step_index[sl].to(device)
            acc.update([torch.zeros(1, device=device)] + outs, [torch.zeros(1, device=device)] + tgts, step_index=si)
    return acc


def check_result_against_golden(case, res):
    for h, (name, C, _, n_names) in enumerate(case.heads):
        r = res[name]
        assert r['confusion'].dtype == np.int64 and np.array_equal(r['confusion'], case.want(h, 'counts')), (case.name, h)
        report = pp.classification_report(r['confusion'], head_names(case, h), output_dict=True)
        check_metrics(case, h, r['micro'], r['macro'], report)
        # the accumulator's own report is over range(C); its class rows are the named rows of the count matrix
        assert close([r['report'][str(c)]['support'] for c in range(C)], case.want(h, 'counts').sum(1))
        yt, yp = case.want(h, 'targets'), case.want(h, 'labels')
        steps = yt.shape[1]
        seq_t, seq_p = yt.transpose(0, 2, 1).reshape(-1, steps), yp.transpose(0, 2, 1).reshape(-1, steps)
        for ov, recorded in zip(OVERLAPS, case.want(h, 'f1_at_k')):
            got = r['f1@k'][ov]
            if (seq_t == -1).all():
                assert math.isnan(got) and np.isnan(recorded)
                continue
            want = R.f1_at_k(seq_t, seq_p, C, ov, ignore_value=-1.0)
            assert abs(got - want) < 1e-6, (case.name, h, ov, got, want)
            if n_names == C:                               # the reference's own figure (its num_classes = len(names))
                assert abs(got - recorded) < 1e-6, (case.name, h, ov, got, recorded)


def check_host_layer_against_golden(device):
    for case in cases():
        check_result_against_golden(case, run_accumulator(case, device).result())
        # the dict-of-labels route: process_output-style labels -> evaluate_predictions / the label-level mirrors
        labels = {h[0]: torch.from_numpy(case.want(i, 'labels')).to(device) for i, h in enumerate(case.heads)}
        truths = {h[0]: torch.from_numpy(case.want(i, 'targets')).to(device) for i, h in enumerate(case.heads)}
        sub = next((head_names(case, i) for i, h in enumerate(case.heads) if 'affordance' not in h[0]), None)
        aff = next((head_names(case, i) for i, h in enumerate(case.heads) if 'affordance' in h[0]), None)
        res = pp.evaluate_predictions(truths, labels, print_report=False, subactivity_names=sub, affordance_names=aff)
        for i, h in enumerate(case.heads):
            for average in ('micro', 'macro'):
                got = res[f'{h[0]}-{average}']
                assert close([got['precision'], got['recall'], got['f1']], case.want(i, average)), (case.name, i, average)


def test_host_layer_matches_reference_golden(fake_backend):
    check_host_layer_against_golden('cpu')


def check_label_level_mirrors(device):
    """downsample_bad_bimanual_videos / summarize_frames_into_segments on plain labels (what predict_labels gives for every
    target step) end with the labels and targets the reference's pipeline ends with."""
    for case in cases():
        if case.step_index is None:
            continue
        plain_l, plain_t = {}, {}
        for h, (name, *_rest) in enumerate(case.heads):
            logp, tgt = case.batches[0][h]
            plain_l[name] = torch.from_numpy(R.predict_labels(logp, case.ds, tgt.shape[1])).to(device)
            plain_t[name] = torch.from_numpy(tgt).to(device)
        if 'bimanual' in case.name:
            got_l, got_t = pp.downsample_bad_bimanual_videos(plain_l, plain_t, case.z[f'{case.name}_is_15fps'])
        else:
            starts = [[int(s) for s in row if s >= 0] for row in case.z[f'{case.name}_segment_starts']]
            got_l = pp.summarize_frames_into_segments(plain_l, starts, is_ground_truth=False)
            got_t = pp.summarize_frames_into_segments(plain_t, starts, is_ground_truth=True)
        for h, (name, *_rest) in enumerate(case.heads):
            assert np.array_equal(got_l[name].cpu().numpy(), case.want(h, 'labels')), (case.name, h)
            assert np.array_equal(got_t[name].cpu().numpy(), case.want(h, 'targets')), (case.name, h)


def test_label_level_mirrors_match_reference_golden():
    check_label_level_mirrors('cpu')


def test_half_rate_step_index():
    got = pp.half_rate_step_index(5, [False, True]).numpy()
    assert got.dtype == np.int32 and got.tolist() == [[0, 1, 2, 3, 4], [1, 3, -1, -1, -1]]
    assert pp.half_rate_step_index(4, [True]).numpy().tolist() == [[1, 3, -1, -1]]
    assert pp.segment_step_index([[0, 2], [0], [0, 1, 5]]).numpy().tolist() == [[0, 2, -1], [0, -1, -1], [0, 1, 5]]


@pytest.mark.parametrize('splits', [1, 2, 5])
def test_accumulator_is_independent_of_the_batch_partition(fake_backend, splits):
    for case in cases():
        check_result_against_golden(case, run_accumulator(case, 'cpu', splits=splits).result())


def test_result_raises_on_out_of_range_target(fake_backend):
    case = cases()[0]
    name, C = case.heads[0][0], case.heads[0][1]
    logp, tgt = case.batches[0][0]
    bad = tgt.copy()
    bad[0, 0, 0], bad[1, 1, 0] = C, -2
    acc = pp.EvaluationAccumulator([name], C)
    acc.update([torch.from_numpy(logp)], [torch.from_numpy(bad)])
    with pytest.raises(ValueError, match=rf"{name}.*\b2 evaluated positions"):
        acc.result()
    acc = pp.EvaluationAccumulator([name], C)
    si = torch.tensor([[0, tgt.shape[1], -1]] * logp.shape[0], dtype=torch.int32)
    acc.update([torch.from_numpy(logp)], [torch.from_numpy(tgt)], step_index=si)
    with pytest.raises(ValueError, match=rf'{name}.*\b{logp.shape[0] * logp.shape[3]} evaluated positions have a step_index'):
        acc.result()
    with pytest.raises(ValueError, match='1 evaluated positions'):
        pp.evaluate_predictions({name: torch.tensor([[0, 1, -3]])}, {name: torch.tensor([[0, 1, 1]])}, print_report=False)


def test_more_classes_than_the_histogram_holds_raises(fake_backend):
    acc = pp.EvaluationAccumulator(['x'], 65)
    with pytest.raises(RuntimeError):
        acc.update([torch.zeros(1, 65, 2, 1)], [torch.zeros(1, 2, 1, dtype=torch.int64)])


def test_print_report_names_every_class(fake_backend):
    case = next(c for c in cases() if c.name == 'cad120')
    labels = {h[0]: torch.from_numpy(case.want(i, 'labels')) for i, h in enumerate(case.heads)}
    truths = {h[0]: torch.from_numpy(case.want(i, 'targets')) for i, h in enumerate(case.heads)}
    sub = [f'subactivity-{i}' for i in range(10)]
    aff = [f'affordance-{i}' for i in range(12)]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        pp.evaluate_predictions(truths, labels, print_report=True, subactivity_names=sub, affordance_names=aff)
    text = buf.getvalue()
    for n in sub + aff:
        assert n in text.split(), n
    for heading in ('Sub-activity Recognition', 'Sub-activity Prediction', 'Affordance Recognition', 'Affordance Prediction',
                    'accuracy', 'macro avg', 'weighted avg'):
        assert heading in text, heading
    # the table shows the numbers of the dict form
    rep = pp.classification_report(case.want(0, 'counts'), sub, output_dict=True)
    assert f'{rep["macro avg"]["f1-score"]:.4f}' in text


def _rank_worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    twog_kernels._set_backend_for_tests(EvaluationFakeKernels())
    torch.set_num_threads(2)
    out = {}
    for case in cases():
        acc = pp.EvaluationAccumulator([h[0] for h in case.heads], [h[1] for h in case.heads], downsampling=case.ds,
                                       overlaps=OVERLAPS)
        for batch in case.batches:                          # every rank takes its half of the clips of every batch
            bs = batch[0][0].shape[0]
            part = np.array_split(np.arange(bs), world)[rank]
            sl = slice(int(part[0]), int(part[-1]) + 1)
            si = None if case.step_index is None else case.step_index[sl]
            acc.update([torch.from_numpy(lp[sl]) for lp, _ in batch], [torch.from_numpy(t[sl]) for _, t in batch], step_index=si)
        acc.all_reduce()
        res = acc.result()
        out[case.name] = {n: (r['confusion'], r['micro'], r['macro'], r['f1@k']) for n, r in res.items()}
    ret[rank] = out
    dist.destroy_process_group()


def test_two_rank_all_reduce_matches_single_process(fake_backend):
    port = 33500 + os.getpid() % 2000
    ret = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(2, port, ret), nprocs=2, join=True)
    for case in cases():
        whole = run_accumulator(case, 'cpu').result()
        for rank in (0, 1):
            for name, (confusion, micro, macro, f1) in ret[rank][case.name].items():
                w = whole[name]
                assert np.array_equal(confusion, w['confusion']), (case.name, rank, name)
                assert close(list(micro.values()), list(w['micro'].values()))
                assert close(list(macro.values()), list(w['macro'].values()))
                assert close(list(f1.values()), list(w['f1@k'].values())), (f1, w['f1@k'])   # fp64 sums of the same fp32 terms
        # and the whole-set result is the golden's
        check_result_against_golden(case, whole)


def test_cross_check_against_live_scikit_learn():
    """An extra: G15 is the pin (scikit-learn may be absent where the suite runs)."""
    metrics = pytest.importorskip('sklearn.metrics')
    import warnings
    rng = np.random.RandomState(3)
    for C, n_names, n in ((7, 7, 400), (9, 5, 300), (3, 3, 5), (6, 8, 50)):
        yt, yp = rng.randint(0, C, size=n), rng.randint(0, C, size=n)
        yp[: n // 2] = yt[: n // 2]
        counts, _ = E.confusion_counts(yt, yp, C)
        names = [f'n{i}' for i in range(n_names)]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for average in ('micro', 'macro'):
                p, r, f, _ = metrics.precision_recall_fscore_support(yt, yp, average=average)
                got = pp.precision_recall_f1(counts, average)
                assert close([got['precision'], got['recall'], got['f1']], [p, r, f]), (C, average)
            want = metrics.classification_report(yt, yp, labels=list(range(n_names)), target_names=names, output_dict=True)
        got = pp.classification_report(counts, names, output_dict=True)
        assert set(got) == set(want)
        for k, v in want.items():
            if isinstance(v, dict):
                assert close([got[k][m] for m in ('precision', 'recall', 'f1-score', 'support')],
                             [v[m] for m in ('precision', 'recall', 'f1-score', 'support')]), (C, k)
            else:
                assert close(got[k], v)
