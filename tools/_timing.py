"""What the ``bench_*.py`` tools of the learner's entry points share: one call between two device events, alternating series, the
median and the deciles, and the emitter that prints a line, keeps it and writes ``--out``."""
import os
import statistics

import torch


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # microseconds


def series(fns, reps, warm):
    """``reps`` timed rounds over ``fns`` in their order (the paths alternate call by call) after ``warm`` untimed ones: one list per path."""
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for f, o in zip(fns, out):
            o.append(one(f))
    return out


def stats(xs):
    """(median, first decile, ninth decile)."""
    xs = sorted(xs)
    return statistics.median(xs), xs[len(xs) // 10], xs[(9 * len(xs)) // 10]


class Emitter:
    """``emit(text)`` prints the line and keeps it; ``close()`` writes the lines to ``path`` (None: nowhere).  ``as_it_grows`` writes the file
    after every line, so that a case that fails leaves the earlier ones."""

    def __init__(self, path=None, as_it_grows=False):
        self.path, self.as_it_grows, self.lines = path, as_it_grows, []

    def __call__(self, text):
        print(text, flush=True)
        self.lines.append(text)
        if self.as_it_grows:
            self.close()

    def close(self):
        if self.path:
            os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
            with open(self.path, "w") as fh:
                fh.write("\n".join(self.lines) + "\n")
