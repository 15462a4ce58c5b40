"""Times the routes of include/pgh_select.h against what they replace, on one GPU.

    python tools/select_lists_bench.py --scale 20 --columns 64 --k 100 [--log profiles/select/<name>.log]

Pairs (each the median of 9 runs, the two routes alternating, min..max beside it; wall clock around calls that end synchronised):
  top       DeviceMatrix.top(k) on a [2^scale, columns] slab  |  slab.numpy(), then argpartition and a lexsort of the k kept per column
  subgraph  Subgraph.transform + Supergraph.transform of a signal with k non-zeros on an AdjacencyWrapper  |  the same with fused = False
            (the host mirror: all n values come down, n zeros go up); the scipy slicing of the adjacency is part of both
  mabs      MabsMaintain().propagate on the slab, route "slab"  |  fused = False, route "columns"
  separate  SeparateNormalization(separator).propagate, route "slab"  |  fused = False, route "columns"
One JSON line per pair goes to stdout and, with --log, to the file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = 9


def timed(routes, sync):
    """{name: (median, min, max) in ms} of the callables in `routes`, run in turn RUNS times after one warm-up each."""
    times = {name: [] for name in routes}
    for name, run in routes.items():
        run()
    sync()
    for _ in range(RUNS):
        for name, run in routes.items():
            start = time.perf_counter()
            run()
            sync()
            times[name].append((time.perf_counter() - start) * 1e3)
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def host_top(slab, k):
    """What a user does without the entry: download, argpartition, order the k kept."""
    values = slab.numpy()
    n, b = values.shape
    rows = np.empty((k, b), dtype=np.int32)
    for j in range(b):
        column = values[:, j]
        kept = np.argpartition(-column, k - 1)[:k] if k < n else np.arange(n)
        cut = column[kept].min()
        kept = np.flatnonzero(column >= cut)                           # every row that ties with the cut, so that ties go by row
        rows[:, j] = kept[np.lexsort((kept, -column[kept]))[:k]]
    return rows, np.take_along_axis(values, rows.astype(np.int64), axis=0)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--scale", type=int, default=20)
    parser.add_argument("--columns", type=int, default=64)
    parser.add_argument("--k", type=int, default=100)
    parser.add_argument("--log", default=None)
    args = parser.parse_args()
    import pygrank_amd as pg
    from pygrank_amd import _lib as L
    pg.load_backend("hip")
    n, b, k = 1 << args.scale, args.columns, args.k
    rng = np.random.default_rng(0)
    sync = lambda: L.check(L.lib().pgh_sync())                       # noqa: E731
    lines = []

    def report(pair, figures, **extra):
        line = dict(pair=pair, scale=args.scale, columns=b, k=k, runs=RUNS, device=L.runtime_name(), **extra)
        for name, (median, low, high) in figures.items():
            line[name + "_ms"] = dict(median=round(median, 3), min=round(low, 3), max=round(high, 3))
        names = list(figures)
        line["ratio"] = round(figures[names[1]][0] / figures[names[0]][0], 2)     # the replaced route's time over the engine route's
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    slab = pg.DeviceMatrix.from_host(rng.random((n, b)).astype(np.float32).astype(np.float64))
    got, want = slab.top(k), host_top(slab, k)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    report("top", timed({"engine": lambda: slab.top(k), "download": lambda: host_top(slab, k)}, sync), slab_mb=round(n * b * 4 / 2 ** 20, 1))

    adjacency = sp.random_array((n, n), density=8.0 / n, format="csr", random_state=np.random.default_rng(1), dtype=np.float64)
    graph = pg.AdjacencyWrapper(adjacency, directed=True)
    values = np.zeros(n)
    values[rng.choice(n, size=min(k, n), replace=False)] = 1.0 + rng.random(min(k, n))
    signal = pg.to_signal(graph, values)

    def there_and_back(fused):
        down, up = pg.Subgraph(), pg.Supergraph()
        down.fused = up.fused = fused
        signal._host = None                                           # a fresh signal has no mirror yet
        return up.transform(down.transform(signal))
    assert np.array_equal(np.asarray(there_and_back(True).np), np.asarray(there_and_back(False).np))
    report("subgraph", timed({"engine": lambda: there_and_back(True), "mirror": lambda: there_and_back(False)}, sync))

    separator = pg.to_signal(graph, (rng.random(n) < 0.4).astype(np.float64))
    for pair, make in (("mabs", lambda: pg.MabsMaintain()), ("separate", lambda: pg.SeparateNormalization(separator))):
        def run(fused, route):
            post = make()
            post.fused = fused
            out = post.propagate(graph, slab)
            assert post.last_propagate["route"] == route
            return out
        report(pair, timed({"slab": lambda: run(True, "slab"), "columns": lambda: run(False, "columns")}, sync))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as handle:
            handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
