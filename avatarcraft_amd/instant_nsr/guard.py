"""The NaN guard of the training renders: a flag per render behind an event, looked at later, never waited for on the hot path."""
import math

import torch


class FiniteGuard:
    """what NeRFRenderer inherits; plain functions on `self.__dict__` (a data-parallel step borrows them into a class of its own)"""

    # The reference stops a training render on a NaN normal (`assert (gradient == gradient).all()`, instant_nsr.py:274), which costs it a host
    # round trip per render.  Here every training render leaves a one-word "gradient_error is not finite" flag in pinned host memory behind an
    # event; the flags of earlier renders are looked at (never waited for) on the next one, and check_finite() waits for all of them.
    # The step functions (stylize.sds_step, reconstruct.reconstruct_step) call check_finite() BEFORE optimizer.step(): the event is recorded right
    # behind the training forward, i.e. it has fired long before the host gets there (the backward is still queued), so a poisoned gradient raises
    # before Adam's state or the weights are touched -- the reference's order (assert, then backward, then step).  A caller that drives
    # render() + its own optimizer gets the flag on its next render, on check_finite(), or when the net is pickled / checkpointed / deep-copied.
    # nan_guard = False switches it off.
    nan_guard = True

    def _guard_finite(self, gerr):
        # a data-parallel step is collecting (stylize._collective_verdict): the flag is NOT judged on this rank -- neither now nor by a later render's
        # non-waiting poll (a rank whose patch k produced NaN raised inside patch k + 1's render, before the gradient collective, and the
        # healthy ranks hung in the all-reduce) -- it is folded into the guard word of the step's collective, whose verdict every rank sees
        defer = self.__dict__.get("_nan_deferred")
        if defer is not None:
            if self.nan_guard and isinstance(gerr, torch.Tensor):
                defer.append(gerr.detach().reshape(-1)[:1].float())
            return
        if not self.nan_guard or not isinstance(gerr, torch.Tensor) or not gerr.is_cuda:
            if self.nan_guard and isinstance(gerr, torch.Tensor) and not bool(torch.isfinite(gerr).all()):
                raise FloatingPointError("NaN / Inf in the finite-difference normals of a training render (reference: instant_nsr.py:274)")
            return
        pend = self.__dict__.setdefault("_nan_pending", [])
        self._poll_finite(wait=False)
        host = torch.zeros(1, dtype=torch.float32).pin_memory()      # the value itself travels (one 4-byte copy, no kernel); it is judged on the host
        host.copy_(gerr.detach().reshape(1), non_blocking=True)
        ev = torch.cuda.Event(); ev.record()
        pend.append((ev, host))

    def _poll_finite(self, wait):
        pend = self.__dict__.get("_nan_pending", [])
        while pend and (wait or pend[0][0].query()):
            ev, host = pend.pop(0)
            ev.synchronize()
            if not math.isfinite(float(host[0])):
                pend.clear()
                raise FloatingPointError("NaN / Inf in the finite-difference normals of a training render (reference: instant_nsr.py:274)")

    def check_finite(self):
        """wait for the NaN flags of every training render issued so far; raises FloatingPointError if one of them was set"""
        self._poll_finite(wait=True)
