"""What every tools/*_bench.py shares, once: the bring-up of the engine, the seeded workload, the event timer, the alternating sampler,
the summary of its samples, the disjoint-spreads rule and the one-line record.

The method the tools' figures rest on (README, the tools): ONE process; the routes compared run in turn inside every round, in the
order the tool names them; one warm-up round of every route (code objects, pooled blocks, plans) that is not counted; `reps` timed
rounds; the median with min..max; a route counts as faster only when the two min..max intervals do not overlap.  `Timer` reads
pgh_timer_* -- events on the engine's stream, host work between the launches included.

No main, and nothing of the package is imported before a function here is called.
"""
import ctypes as C
import json
import os
import statistics

import numpy as np


class Timer:
    def __init__(self, L):
        self.L, self.lib, self.h = L, L.lib(), L.c_timer()
        L.check(self.lib.pgh_timer_create(C.byref(self.h)))

    def time(self, fn):
        self.L.check(self.lib.pgh_timer_start(self.h))
        value = fn()
        self.L.check(self.lib.pgh_timer_stop(self.h))
        ms = C.c_double()
        self.L.check(self.lib.pgh_timer_elapsed_ms(self.h, C.byref(ms)))
        return ms.value, value


def summary(samples):
    return dict(median_ms=round(statistics.median(samples), 4), min_ms=round(min(samples), 4), max_ms=round(max(samples), 4),
                samples=len(samples))


def disjoint(a, b, lo="min_ms", hi="max_ms"):
    """Whether the min..max intervals of two summaries do not overlap (touching intervals overlap)."""
    return bool(a[hi] < b[lo] or b[hi] < a[lo])


def over(a, b, places=4):
    """The ratio of two summaries' medians."""
    return round(a["median_ms"] / b["median_ms"], places)


def sample(timer, routes, reps, each=None, keep=True):
    """({name: [ms] * reps}, {name: last value}) of the callables in `routes`, which run in dict order inside every round.  The first
    round warms every code object and pooled block up and is not kept.  `each(name, value)` is called after every run, that round's
    included, outside the timed region.  What a run returns stays alive until the same route has run again; with keep=False only until
    the next run of any route has ended (and only the very last value is handed out).  It matters when the values own device memory:
    a route whose previous result is still alive gets other blocks from the pool (4 % of a 0.43 ms slab pass at scale 20)."""
    samples, last = {name: [] for name in routes}, {}
    for rep in range(reps + 1):
        for name, once in routes.items():
            ms, value = timer.time(once)
            if not keep:
                last.clear()
            last[name] = value
            if each is not None:
                each(name, last[name])
            if rep:
                samples[name].append(ms)
    return samples, last


def alternate(timer, routes, reps, each=None, keep=True):
    """`sample`, every route's milliseconds summarised: ({name: summary}, {name: last value})."""
    samples, last = sample(timer, routes, reps, each, keep)
    return {name: summary(got) for name, got in samples.items()}, last


def engine(*entries, what=None):
    """(pg, L, Timer(L)) with the hip backend loaded and the device initialised (which raises without an MI355X); SystemExit when the
    engine library lacks one of `entries`, named by `what` or by the first entry that is missing."""
    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    pg.load_backend("hip")
    L.ensure_init()
    for name in entries:
        if L.entry(name) is None:
            raise SystemExit("the engine library lacks " + (what or name))
    return pg, L, Timer(L)


def rmat(args, **kw):
    """The tools' RMAT graph, built on the device: --scale, --ef, seed 0, the Graph500 quadrant weights."""
    from pygrank_amd.synthetic import rmat_graph
    return rmat_graph(args.scale, args.ef, seed=0, a=0.57, b=0.19, c=0.19, **kw)


def nodes_with_edges(pg, adj):
    return np.flatnonzero(np.asarray(pg.degrees(adj.array)) > 0)


def seed_vector(n, nodes, seeds, rng):
    """A host indicator of `seeds` of `nodes` (all of them when there are fewer), one `rng.choice` without replacement."""
    p = np.zeros(n)
    p[rng.choice(nodes, size=min(seeds, len(nodes)), replace=False)] = 1.0
    return p


def seed_columns(pg, n, nodes, width, seeds, rng):
    """`width` seed vectors, drawn one after the other, as device columns."""
    return [pg.DeviceVector.from_host(seed_vector(n, nodes, seeds, rng)) for _ in range(width)]


def emit(record, path=None):
    """The record as one JSON line on stdout and, with `path`, as that file's content (its directory is created)."""
    line = json.dumps(record)
    print(line, flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
