"""The guard every stream capture of this package runs under (``Environment.capture_turn``, ``PyTorchIQN.capture_train_step``)."""
from __future__ import annotations

import contextlib
import gc

import torch


@contextlib.contextmanager
def recording(graph: "torch.cuda.CUDAGraph"):
    """``with recording(graph): body`` records ``body``'s launches on the current device into ``graph`` (``torch.cuda.graph``).

    No garbage collection inside the capture: an unreachable engine or graph of an EARLIER environment that the collector happens to
    free now would call hipFree / hipGraphDestroy while a stream is capturing, which HIP forbids -- the capture fails, and torch aborts
    the process while it unwinds (seen under rocprofv3, where the timing differs; torch.cuda.graph no longer collects on entry itself).
    The window: process-wide and NOT thread-safe (another thread that re-enables the collector, or drops the last reference to an engine /
    graph between here and the end of the capture, still frees inside it) -- a capture is a single-threaded moment of the caller's program.
    Reference-counted frees of THIS thread are kept out explicitly: engines whose close() is pending are closed now, before the capture,
    and those that became pending during it once it has ended."""
    from sorrel_amd.engine import GridEngine

    gc.collect()
    GridEngine.drain_pending_closes()
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            yield graph
    finally:
        if gc_was_on:
            gc.enable()
    GridEngine.drain_pending_closes()
