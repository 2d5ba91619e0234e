"""Admission and failure handling of the persistent launches: plain Python over device indices, a launch's
return code and its error word. No ctypes, no library, no device: kernels.py supplies the launches and the read-backs.

The persistent launches need every workgroup of their grid resident at once. Three lines of defence:
 (1) a device this process shares with other ranks of its own group (distributed.DataParallel finds out at construction:
     more ranks than devices) is listed in `shared_devices` and never gets a persistent launch;
 (2) the library asks the runtime's occupancy figure before launching and refuses a grid the device cannot hold (rc
     TWOG_PERSIST_NOT_RESIDENT);
 (3) a tenant nobody told us about (another process, another stream's long kernel, a CU mask): every wait inside the
     launch is bounded, a time-out sets the launch's error word and drains the grid; the host reads the word and re-runs
     the pass on the launch-per-step path -- same buffers, written in place. A device on which that happened gets no
     persistent launches for the next BACKOFF calls.

When is the error word read? Reading it right after the launch is one 4-byte read-back, but it drains the stream while
the host waits (about one launch latency), and the host then has to refill the queue launch by launch (measured at 8
clips: ~0.4 ms of the 21.5 ms step per read-back). So: the first SYNC_CALLS persistent launches on a device -- and every
launch after a failure, until as many have completed again -- are checked AT ONCE and recovered transparently (the pass
is re-run per step before anything consumes its outputs). After that many clean launches the device is evidently ours:
the word is copied to pinned host memory behind the launch (asynchronously) and read at the END of the forward / backward
pass (verify, called by ops.tggcn_forward / tggcn_backward through kernels.verify_persistent), when the copy has long
landed. A failure found that late -- a tenant that arrived in mid-training -- cannot be repaired behind the caller's back
(consumers have run on incomplete outputs): it raises, loudly, with the process and the context alive, and the next calls
are checked at once again. TWOG_PERSIST_CHECK=sync: always at once; =lazy: always at the end of the pass.
"""
import os

PERSIST_NOT_RESIDENT = -3   # TWOG_PERSIST_NOT_RESIDENT (= _lib.PERSIST_NOT_RESIDENT; tests/test_persist_policy_cpu.py)


class PersistentLaunches:
    """One instance per process (kernels.PERSIST); every index `i` is a device index of this process."""

    BACKOFF = 64     # calls without persistent launches after one gave up
    SYNC_CALLS = 8   # clean launches checked at once before the check moves to the end of the pass

    def __init__(self):
        self.shared_devices = set()   # device indices: ranks of one group share them
        self.backoff = {}             # device index -> calls left without persistent launches
        self.clean = {}               # device index -> persistent launches checked at once that completed
        self.refused = set()          # keys (launch, device index, shape ...) the occupancy check refused: not asked again
        self.pending = {}             # device index -> [deferred check: .what, .value() waits and returns the error word]
        self.fallbacks = 0            # passes re-run on the launch-per-step path after a persistent launch gave up
        self.refusals = 0             # persistent launches the occupancy check refused
        self.late_failures = 0        # passes whose failure was found at their end

    def blocked(self, i, key=None):
        """Whether a persistent launch on device i (of the grid `key`) would be turned down. Consumes nothing: for callers
        that plan around the answer before the launch is attempted."""
        return i in self.shared_devices or self.backoff.get(i, 0) > 0 or (key is not None and key in self.refused)

    def allowed(self, i):
        """False on a shared device, and for BACKOFF calls after a persistent launch on this device gave up: each such call
        consumes one, so ask last, for a launch that would otherwise be attempted."""
        if i in self.shared_devices:
            return False
        left = self.backoff.get(i, 0)
        if left > 0:
            self.backoff[i] = left - 1
            return False
        return True

    def _gave_up(self, i):
        self.backoff[i] = self.BACKOFF
        self.clean[i] = 0

    def completed(self, i, rc, what, read_now, defer, key=None):
        """After the launch `what` returned rc: True if it ran to completion (or will be verified at the end of the pass),
        False -> the caller re-runs the pass on the launch-per-step path. read_now() drains the stream and returns the error
        word; defer() enqueues its copy and returns the deferred check. A refused grid is remembered under `key`, if given."""
        if rc == PERSIST_NOT_RESIDENT:
            self.refusals += 1
            if key is not None:
                self.refused.add(key)
            return False
        if rc != 0:
            raise RuntimeError(f'{what} failed with code {rc}')
        mode = os.environ.get('TWOG_PERSIST_CHECK', 'auto')
        if mode == 'lazy' or (mode != 'sync' and self.clean.get(i, 0) >= self.SYNC_CALLS):
            self.pending.setdefault(i, []).append(defer())
            return True
        if read_now() == 0:
            self.clean[i] = self.clean.get(i, 0) + 1
            return True
        self.fallbacks += 1
        self._gave_up(i)
        return False

    def verify(self, i):
        """End of a forward / backward pass: every persistent launch of the pass whose error word was left for later must
        have completed. Raises RuntimeError otherwise, once."""
        failed = [d.what for d in self.pending.pop(i, ()) if d.value() != 0]
        if failed:
            self.late_failures += 1
            self._gave_up(i)
            raise RuntimeError(f'{", ".join(failed)}: a persistent launch could not keep its grid resident (another tenant '
                               'is holding compute units of this GPU) and gave up; the results of this pass are incomplete. '
                               'Repeat the step: the next calls run the launch-per-step path and persistent launches are '
                               're-admitted one checked launch at a time (TWOG_BIGRU_PERSIST=0 TWOG_SEG_PERSIST=0 switch '
                               'them off for good).')
