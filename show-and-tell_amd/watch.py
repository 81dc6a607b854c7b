"""Device-side status words, read back without stalling the stream: `StatusRing` copies a word to pinned host memory behind the call
that may set it, and looks at it later, oldest first.  `ResidencyWatch` watches kernels that need ALL their workgroups resident
at once (the persistent LSTM recurrence, `sat_lstm_persist.hip`; the fused conv3 + BatchNorm + add + ReLU launch with its grid-wide
statistics barrier, `sat_conv3_fused.hip`).  Every wait inside such a kernel is bounded; when one runs out (co-tenants on the
device kept part of the grid from being scheduled) the kernel sets a sticky status word and leaves -- the outputs of that call
are garbage.  That must never pass silently: the word is looked at when the next call is submitted (or at once with
`poll(block=True)`; `TrainStep.check_ids()` does); non-zero raises RuntimeError after the caller's `on_error` hook has switched
the process to the form that needs no co-residency.  `IdGuard` checks caption ids the same way."""
import torch

from . import _lib as L


class StatusRing:
    """Pinned int32 ring, one slot and one event per status word in flight."""

    def __init__(self, depth):
        self.host = torch.zeros(depth, dtype=torch.int32).pin_memory()
        self.pending = []           # (slot, event, payload), oldest first
        self.slot = 0

    def push(self, word, payload):
        """word: a 1-element int32 device view, copied behind the work enqueued so far on the current stream"""
        slot = self.slot
        self.slot = (slot + 1) % self.host.numel()
        self.host[slot:slot + 1].copy_(word, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((slot, ev, payload))

    def retire(self, block, keep=0):
        """Look at the words in flight, oldest first, until `keep` are left (not blocking: or one is not copied yet).  Returns
        (code, payload) of the first non-zero word -- the ring is then emptied -- or None."""
        while len(self.pending) > keep:
            slot, ev, payload = self.pending[0]
            if block:
                ev.synchronize()
            elif not ev.query():
                return None
            self.pending.pop(0)
            code = int(self.host[slot])
            if code != 0:
                self.host.zero_()
                self.pending.clear()
                return code, payload
        return None


class ResidencyWatch:
    DEPTH = 16
    _by_device = {}

    @classmethod
    def get(cls, device):
        key = str(device)
        w = cls._by_device.get(key)
        if w is None:
            w = cls._by_device[key] = cls()
        return w

    def __init__(self):
        self.ring = StatusRing(self.DEPTH)

    # what an exception says about the model's state when the caller gave no note of its own: the status word is seen one call
    # later at the latest, and whatever consumed the call's outputs in between -- a torch optimizer step after
    # `loss.backward()` -- has used them.  `trainer.TrainStep` gates its update on the device instead and says so.
    DEFAULT_NOTE = ("the outputs of that call are invalid, and anything computed from them since -- an optimizer step taken "
                    "after loss.backward() included -- has used them: restore the parameters from a checkpoint")

    def submit(self, word, what, on_error=None, note=None):
        """word: a 1-element int32 device view of the status word the call that was just enqueued on the current stream may set;
        note: what the exception tells the user about parameters / optimizer state (DEFAULT_NOTE)"""
        self._raise(self.ring.retire(block=False))
        self._raise(self.ring.retire(block=True, keep=self.DEPTH - 1))
        self.ring.push(word, (what, on_error, note))

    def _raise(self, fault):
        if fault is None:
            return
        code, (what, on_error, note) = fault
        torch.cuda.synchronize()
        if on_error is not None:
            on_error()
        raise RuntimeError("show-and-tell_amd: %s timed out waiting for its workgroups to be resident together (status 0x%x: other "
                           "work shares the device); %s.  Later calls use the form without a device-wide wait"
                           % (what, code & 0xffffffff, note or self.DEFAULT_NOTE))

    def poll(self, block=False):
        self._raise(self.ring.retire(block))


class IdGuard:
    """Out-of-range caption ids.  `nn.Embedding` (models.py:49) and `nn.CrossEntropyLoss` (train.py:143) raise on an id
    outside [0, V); the gather / CE kernels here clamp such ids for memory safety only, so every batch is range-checked
    on the device (`sat_validate_ids`, one tiny launch) and the verdict is read back WITHOUT stalling the stream: the
    status word is copied to pinned host memory behind the check and looked at when the next batch is submitted (or
    at once with `poll(block=True)`).  A corrupt caption therefore raises at the latest one step later."""

    DEPTH = 4     # verdicts in flight: the host may run this many submits ahead of the GPU without waiting

    def __init__(self, device):
        self.status = torch.zeros(1, dtype=torch.int32, device=device)       # sticky: only a raise clears it
        self.ring = StatusRing(self.DEPTH)

    def submit(self, ids, ncols, V, what):
        self.poll(block=False)
        if ids.dim() != 2 or ids.dtype != torch.int64 or ids.stride(1) != 1:
            raise TypeError("%s must be an int64 matrix with contiguous rows" % what)
        self._raise(self.ring.retire(block=True, keep=self.DEPTH - 1))
        L.check(L.load().sat_validate_ids(ids.data_ptr(), ids.stride(0), ids.shape[0], min(int(ncols), ids.shape[1]), 0, int(V),
                                          self.status.data_ptr(), L.stream()), "sat_validate_ids")
        self.ring.push(self.status, "%s: id outside [0, %d)" % (what, V))

    def _raise(self, fault):
        if fault is None:
            return
        torch.cuda.current_stream().synchronize()
        self.status.zero_()
        raise IndexError("show-and-tell_amd: %s (nn.Embedding / CrossEntropyLoss would raise here: "
                         "models.py:49, train.py:143)" % fault[1])

    def poll(self, block=False):
        self._raise(self.ring.retire(block))
