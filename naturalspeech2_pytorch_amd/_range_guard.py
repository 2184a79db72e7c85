"""Host side of the IEEE-half range guard (csrc/ns2_common.h `note_out_of_range`): the one place that calls `ns2_saturation_peek` and owns
the pinned words and the event behind them.  WHEN to peek and what a new count means is the callers' policy: `HipDenoiserMixin` (every
few inference forwards, Ns2Error) and the mixed-arithmetic training pass (`_Scale.overflowed`, `GraphedTrainStep.overflowed`)."""
import torch

from . import _lib


class RangePeek:
    """A stream-ordered, non-synchronising copy of a device's range counters into pinned host memory, and the event recorded behind it.
    The order of the words is the library's business: sum them (`total`) or compare them with another peek (`moved`)."""

    def __init__(self):
        self.words = None            # pinned int32[ns2_saturation_counters()], allocated by the first take() and rewritten by later ones
        self.event = None            # recorded behind the copies; None: nothing taken, or the result has been dropped
        self.device = None

    def take(self, device=None):
        """enqueue the copies on `device`'s current stream (None: the current device) and record the event.  Returns self -- or None,
        with nothing enqueued, where there is nothing to peek at: no GPU, no library, a stream under capture."""
        if not torch.cuda.is_available():
            return None
        with torch.cuda.device(device):
            if torch.cuda.is_current_stream_capturing():
                return None
            try:
                lib = _lib.load()
            except Exception:
                return None
            if self.event is not None:
                self.event.synchronize()                 # the pinned words are about to be rewritten
            if self.words is None:
                self.words = torch.zeros(max(lib.ns2_saturation_counters(), 0), dtype=torch.int32).pin_memory()
            _lib.check(lib.ns2_saturation_peek(self.words.data_ptr(), self.words.numel(), torch.cuda.current_stream().cuda_stream),
                       "ns2_saturation_peek")
            self.event = torch.cuda.Event()
            self.event.record()
        self.device = device
        return self

    def in_flight(self):
        return self.event is not None

    def done(self):
        """has the copy arrived?  (no synchronisation)"""
        return self.event is not None and self.event.query()

    def wait(self):
        """wait for the copy, i.e. for the work enqueued before it (one event synchronisation)"""
        self.event.synchronize()

    def total(self):
        return int(self.words.sum().item())

    def drop(self):
        """forget the peek taken: its result has been used, or is no longer wanted"""
        self.event = None


def moved(before):
    """did a range counter of `before`'s device move since `before` (a taken RangePeek, or None)?  Takes a second peek and waits for it --
    for the work enqueued so far.  False when either peek is None."""
    after = None if before is None else RangePeek().take(before.device)
    if after is None:
        return False
    after.wait()
    return bool((after.words != before.words).any().item())
