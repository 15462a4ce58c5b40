"""``Subgraph`` and ``Supergraph`` (pygrank/algorithms/postprocess/subgraph.py:5-68): a signal's non-zero scores move onto the subgraph
their nodes induce, and back.  The reference's README chain runs as written::

    algorithm = pg.PageRank() >> pg.Top(10) >> pg.Threshold() >> pg.Subgraph() >> pg.PageRank() >> pg.Supergraph()

On an ``AdjacencyWrapper`` the selection leaves the device as a list (include/pgh_select.h): pgh_vec_select hands
the ``count`` selected positions to the host and keeps their values in a device vector, which becomes the sub-signal as it stands;
``Supergraph`` is pgh_vec_scatter into a zeroed vector.  Neither downloads the n values nor builds a dictionary.  ``fused = False``, or a
library without the entries, works on the signal's host mirror with the same results.  On networkx-style graphs the selected values are
placed by node name, as in the reference."""
import numpy as np

from pygrank_amd.device import DeviceVector
from pygrank_amd.postprocess import Postprocessor, Tautology
from pygrank_amd.preprocessing import AdjacencyWrapper
from pygrank_amd.signals import GraphSignal, to_signal


class Subgraph(Postprocessor):
    """Extracts the subgraph induced by the non-zero scores and places those scores in a signal on it.  ``graph._pygrank_original_graph``
    of the outcome's graph is the graph the signal came from: what ``Supergraph`` returns to.

    An all-zero signal raises: the subgraph would have no node.  (The reference returns a signal over an empty graph, which no filter can
    rank on.)  A graph that is neither an ``AdjacencyWrapper`` nor has a networkx-style ``subgraph(nodes)`` raises too."""

    def __init__(self, ranker=None):
        super().__init__(Tautology() if ranker is None else ranker)

    def transform(self, ranks, *args, **kwargs):
        graph = ranks.graph
        if not isinstance(graph, AdjacencyWrapper) and not callable(getattr(graph, "subgraph", None)):
            raise Exception("Subgraph needs an AdjacencyWrapper or a graph with a networkx-style subgraph(nodes), not " + type(graph).__name__)
        positions, values = ranks.nonzero(fused=self.fused)
        if len(positions) == 0:
            raise Exception("no non-zero score: the subgraph would be empty")
        if isinstance(graph, AdjacencyWrapper):
            sub = graph.subgraph(positions)
            sub._pygrank_original_graph = graph
            return GraphSignal(sub, values)
        nodes = ranks._nodes_at(positions)
        sub = graph.subgraph(nodes)
        sub._pygrank_original_graph = graph
        return to_signal(sub, dict(zip(nodes, np.asarray(values, dtype=np.float64).tolist())))

    def rank(self, *args, **kwargs):
        return self.transform(self.ranker.rank(*args, **kwargs))

    def propagate(self, graph, features, *args, **kwargs):
        raise Exception("Subgraph has no propagate: every column would live on a subgraph of its own; end the chain with Supergraph")

    def _reference(self):
        return "induced subgraph extraction for non-zero node scores"


class Supergraph(Postprocessor):
    """Returns the scores to the graph ``Subgraph`` departed from, zero on the nodes that were left out.  A chain that ends here may be
    used in ``propagate``: it runs column by column (``last_propagate["route"] == "ranks"``)."""

    def __init__(self, ranker=None):
        super().__init__(Tautology() if ranker is None else ranker)

    def transform(self, ranks, *args, **kwargs):
        graph = ranks.graph
        original = getattr(graph, "_pygrank_original_graph", None)
        if original is None:
            raise Exception("Supergraph: the signal's graph is no outcome of Subgraph (it carries no _pygrank_original_graph)")
        if isinstance(graph, AdjacencyWrapper) and isinstance(original, AdjacencyWrapper):
            positions = graph.original_nodes
            values = ranks.np
            if self.fused and isinstance(values, DeviceVector):
                out = DeviceVector.full(len(original), 0.0)
                if out.scatter(positions, values):
                    return GraphSignal(original, out)
            out = np.zeros(len(original), dtype=np.float64)
            out[positions] = ranks._mirror()
            return GraphSignal(original, out)
        return to_signal(original, {node: ranks[node] for node in ranks})

    def rank(self, *args, **kwargs):
        return self.transform(self.ranker.rank(*args, **kwargs))

    def _reference(self):
        return "returned to subgraph's containing graph"
