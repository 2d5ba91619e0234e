"""The admission and failure-handling policy of the persistent launches (2g-gcn_amd/persist.py) driven on the
CPU: a fresh PersistentLaunches per test, the launch's return code and error word supplied by the test. The GPU tests of
tests/test_kernels_gpu.py make real launches give up; here is the state machine they cannot single out."""
import types

import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib, kernels
from twog_gcn_amd.persist import PERSIST_NOT_RESIDENT, PersistentLaunches


class Rig:
    """One policy object and the two callables kernels.py would supply: read_now() returns `word`, defer() a deferred check
    that returns `word` as it is when the check is waited for. `calls` records which of the two the policy chose."""

    def __init__(self):
        self.P = PersistentLaunches()
        self.word = [0]
        self.calls = []

    def read_now(self):
        self.calls.append('now')
        return self.word[0]

    def defer(self, what):
        self.calls.append('defer')
        return types.SimpleNamespace(what=what, value=lambda: self.word[0])

    def launch(self, i=0, rc=0, what='launch', key=None):
        return self.P.completed(i, rc, what, self.read_now, lambda: self.defer(what), key)

    def state(self):
        P = self.P
        return (set(P.shared_devices), dict(P.backoff), dict(P.clean), set(P.refused), {i: len(v) for i, v in P.pending.items()},
                P.fallbacks, P.refusals, P.late_failures)


@pytest.fixture
def rig(monkeypatch):
    monkeypatch.delenv('TWOG_PERSIST_CHECK', raising=False)
    return Rig()


def test_the_return_code_is_the_one_of_the_binding():
    assert PERSIST_NOT_RESIDENT == _lib.PERSIST_NOT_RESIDENT
    assert kernels.PERSIST.BACKOFF == 64 and kernels.PERSIST.SYNC_CALLS == 8


def test_auto_mode_checks_the_first_launches_of_a_device_at_once_and_defers_afterwards(rig):
    P = rig.P
    for k in range(P.SYNC_CALLS):
        assert rig.launch(0) and P.clean[0] == k + 1
    assert rig.calls == ['now'] * P.SYNC_CALLS and not P.pending
    assert rig.launch(0)
    assert rig.calls == ['now'] * P.SYNC_CALLS + ['defer'] and len(P.pending[0]) == 1 and P.clean[0] == P.SYNC_CALLS
    rig.calls.clear()
    assert rig.launch(1)   # a second device starts from zero
    assert rig.calls == ['now'] and P.clean[1] == 1 and 1 not in P.pending


@pytest.mark.parametrize('mode,clean,want', [('sync', 0, 'now'), ('sync', 1000, 'now'), ('lazy', 0, 'defer'), ('lazy', 1000, 'defer')])
def test_the_check_switch_overrides_the_clean_count(rig, monkeypatch, mode, clean, want):
    monkeypatch.setenv('TWOG_PERSIST_CHECK', mode)
    rig.P.clean[0] = clean
    for _ in range(3):
        assert rig.launch(0)
    assert rig.calls == [want] * 3


def test_a_word_read_at_once_backs_the_device_off_for_backoff_calls(rig):
    P = rig.P
    for _ in range(3):
        rig.launch(0)
    rig.word[0] = 7
    assert rig.launch(0) is False
    assert (P.fallbacks, P.backoff[0], P.clean[0]) == (1, P.BACKOFF, 0) and not P.pending and P.late_failures == 0
    for k in range(P.BACKOFF):
        assert P.blocked(0) and P.blocked(0, ('any', 'key'))
        assert P.backoff[0] == P.BACKOFF - k, 'blocked() lowered the count'
        assert P.allowed(0) is False
        assert P.backoff[0] == P.BACKOFF - k - 1
    assert P.allowed(0) is True and not P.blocked(0) and P.backoff[0] == 0
    assert P.allowed(1) is True, 'another device is not affected'


def test_a_grid_the_device_cannot_hold_is_counted_and_memoised_under_its_key_only(rig):
    P = rig.P
    rig.launch(0)
    before = rig.state()
    assert rig.launch(0, rc=PERSIST_NOT_RESIDENT) is False   # without a key: nothing is memoised
    assert P.refusals == 1 and not P.refused
    key, other = ('bigru_bwd', 0, (2, 4, 1), 8, 512), ('bigru_bwd', 0, (2, 4, 1), 9, 512)
    assert rig.launch(0, rc=PERSIST_NOT_RESIDENT, key=key) is False
    assert P.refusals == 2 and P.refused == {key}
    assert P.blocked(0, key) and not P.blocked(0, other) and not P.blocked(0) and P.allowed(0)
    assert rig.calls == ['now'], 'the error word of a launch that did not happen was asked for'
    assert rig.state()[:3] == before[:3] and rig.state()[4:6] == before[4:6] and P.late_failures == 0   # no back-off, clean untouched


def test_any_other_return_code_raises_naming_the_launch_and_changes_nothing(rig):
    rig.launch(0)
    before = rig.state()
    for rc in (-1, -2, 1, 700):
        with pytest.raises(RuntimeError, match=f'twog_x_persistent failed with code {rc}$'):
            rig.launch(0, rc=rc, what='twog_x_persistent', key=('k',))
    assert rig.state() == before and rig.calls == ['now']


def test_a_shared_device_gets_no_persistent_launch_and_consumes_nothing(rig):
    P = rig.P
    P.shared_devices.add(2)
    assert P.allowed(2) is False and P.blocked(2) and P.backoff == {}
    P.backoff[2] = 5
    assert P.allowed(2) is False and P.backoff[2] == 5
    assert P.allowed(0) and not P.blocked(0)


def test_a_deferred_failure_raises_once_at_the_end_of_the_pass_and_backs_off(rig, monkeypatch):
    P = rig.P
    monkeypatch.setenv('TWOG_PERSIST_CHECK', 'lazy')
    P.clean[0] = 5
    words = {'a': 0, 'b': 3, 'c': 0, 'd': 1}
    for what, w in words.items():
        assert P.completed(0, 0, what, rig.read_now, lambda what=what, w=w: types.SimpleNamespace(what=what, value=lambda: w)) is True
    assert len(P.pending[0]) == 4 and rig.calls == []
    P.verify(1)   # nothing pending there
    with pytest.raises(RuntimeError, match='could not keep its grid resident') as e:
        P.verify(0)
    assert str(e.value).startswith('b, d: a persistent launch')
    assert (P.late_failures, P.fallbacks, P.backoff, P.clean) == (1, 0, {0: P.BACKOFF}, {0: 0}) and not P.pending
    P.verify(0)   # reported once
    assert P.late_failures == 1


def test_deferred_successes_leave_everything_but_pending_alone(rig, monkeypatch):
    P = rig.P
    monkeypatch.setenv('TWOG_PERSIST_CHECK', 'lazy')
    for _ in range(4):
        assert rig.launch(0)
    before = rig.state()
    P.verify(0)
    after = rig.state()
    assert not P.pending and before[4] == {0: 4} and after[:4] == before[:4] and after[5:] == before[5:]


def test_would_persist_asks_for_the_key_the_launch_memoises(monkeypatch):
    """bigru_bwd_would_persist and bigru_bwd build the memo key with one function: what the launch was refused for, the
    question answers no to, and only that."""
    monkeypatch.delenv('TWOG_BIGRU_PERSIST', raising=False)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(kernels, 'PERSIST', PersistentLaunches())
    K = object.__new__(kernels.HipKernels)
    K.lib = types.SimpleNamespace(twog_bigru_bwd_persistent_supported=lambda arr, n, bs, h: 2)
    Es, bs, h = [2, 4, 1], 8, 512
    assert K.bigru_bwd_would_persist(Es, bs, h)
    kernels.PERSIST.refused.add(K._bigru_bwd_key(0, Es, bs, h))
    assert not K.bigru_bwd_would_persist(Es, bs, h)
    assert K.bigru_bwd_would_persist(Es, bs + 1, h)
    kernels.PERSIST.backoff[0] = 1
    assert not K.bigru_bwd_would_persist(Es, bs + 1, h) and kernels.PERSIST.backoff[0] == 1
